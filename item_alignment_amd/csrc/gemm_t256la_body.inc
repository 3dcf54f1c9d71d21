// The body of the T256LA kernels (gemm.hip, namespace t256la), included once per kernel: `p` is the kernel's own argument, ROWS and SLAB
// are compile-time constants of the including kernel.  (Two kernels share this text, not a function: with the body behind a call the
// argument block is copied first and the register allocation of the existing kernels changes.)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane0 = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int nk_all = (p.K + BK - 1) / BK;             // >= 2 (the host sends shorter K to T256W)
  [[maybe_unused]] int n_live = 0;
  if constexpr (ROWS) {
    n_live = __builtin_amdgcn_readfirstlane(p.row_blk[0]);
    p.tiles_m = SLAB ? (n_live + SLAB_TILE - 1) / SLAB_TILE : (n_live + 7) >> 3;
  }
  const int total_tiles = p.tiles_m * p.tiles_n;
  const int n_tiles = nk_all;
  if constexpr (ROWS) {
    if ((int)blockIdx.x >= total_tiles) return;          // fewer live tiles than workgroups
  }
  auto coords = [&](int tile, int& bm, int& bn) { tile_of_index(p, tile, total_tiles, bm, bn); };
  // a tile's operand windows; a tile index past the end gives empty windows: every piece of it reads zeros
  auto window_a = [&](int tile) {
    int bm = 0, bn = 0;
    if (tile < total_tiles) coords(tile, bm, bn);
    return tile < total_tiles ? rsrc_at(p.A, p.a_bytes, ROWS ? (uint64_t)0 : (uint64_t)bm * BM * p.lda) : ia_rsrc(p.A, 0u);
  };
  // ROWS: the row offsets of a tile's eight A pieces (a block the list does not have: the tile's first block once more, never stored)
  auto rows_a = [&](int tile) {
    RowOff ro{};
    if constexpr (ROWS) {
      if (tile < total_tiles) {
        int bm = 0, bn = 0;
        coords(tile, bm, bn);
        if constexpr (SLAB) ro = slab_offsets<false>(p, bm, wave, n_live);
        else {
        const Blk8 bl = load_blk8(p.row_blk, bm, n_live);
#pragma unroll
        for (int j = 0; j < 8; ++j) ro.o[j] = (uint32_t)(bl.b[j] >= 0 ? bl.b[j] : bl.b[0]) * (uint32_t)(32 * p.lda * 2);
        }
      }
    }
    return ro;
  };
  auto window_b = [&](int tile) {
    int bm = 0, bn = 0;
    if (tile < total_tiles) coords(tile, bm, bn);
    return tile < total_tiles ? rsrc_at(p.B, p.b_bytes, (uint64_t)bn * BN * p.ldb) : ia_rsrc(p.B, 0u);
  };

  int lane = lane0;
  asm volatile("" : "+v"(lane));
  const int li = lane & 31;
  const int gt = wave * 64 + lane;
  // ---- DMA lane constants (t256w::main_loop): 8 pieces per operand and k-tile, one lane offset per operand
  const int rowd = gt >> 3;
  const uint32_t voffA = (uint32_t)(((SLAB ? rowd & 7 : rowd) * p.lda + (((gt & 7) ^ ((rowd >> 1) & 7)) * 8)) * 2), stepA = (uint32_t)(32 * p.lda * 2);
  const uint32_t voffB = (uint32_t)((rowd * p.ldb + (((gt & 7) ^ ((rowd >> 1) & 7)) * 8)) * 2), stepB = (uint32_t)(32 * p.ldb * 2);
  const int kl = ((gt & 7) ^ (((gt >> 3) >> 1) & 7)) * 8;          // the k index of this lane's 16 bytes inside a k-tile
  char* const my_part = smem + wave * 1024;
  // ---- fragment addresses
  const int nperm = ((li >> 2) & 1) * 16 + (li >> 3) * 4 + (li & 3);
  uint32_t baseA[4], baseB[4];
  const uint32_t smem_addr = ia_lds_addr(smem);
  frag_bases<false>(baseA, smem_addr, wm * 128, lane, li);
  frag_bases<false>(baseB, smem_addr + TILE_BYTES, wn * 128, lane, nperm);

  int tile = blockIdx.x;
  __amdgpu_buffer_rsrc_t rsA = window_a(tile), rsB = window_b(tile);
  __amdgpu_buffer_rsrc_t rsAn = window_a(tile + (int)gridDim.x), rsBn = window_b(tile + (int)gridDim.x);
  [[maybe_unused]] RowOff roA = rows_a(tile), roAn = rows_a(tile + (int)gridDim.x);

  // k-tile v of the CURRENT tile (v >= n_tiles: k-tile v - n_tiles of the NEXT tile) -> lane offset of its pieces, or out of range
  auto off_of = [&](int v) -> uint32_t {
    const int kt = v >= n_tiles ? v - n_tiles : v;
    return kl < p.K - kt * BK ? 1u : 0u;                 // (1 = in range; the operand's own lane offset is selected by the caller)
  };
  // piece i (0..7: A, 8..15: B) of k-tile v into the buffer at byte offset `buf`
  auto dma = [&](int v, int i, uint32_t ok, uint32_t buf) {
    const bool isB = i >= 8, nx = v >= n_tiles;
    const int j = i & 7, kt = nx ? v - n_tiles : v;
    char* dst = my_part + (isB ? TILE_BYTES : 0) + buf + j * 4096;
    const uint32_t soff = (uint32_t)kt * (uint32_t)(BK * 2) + ((ROWS && !isB) ? (nx ? roAn.o[j] : roA.o[j]) : (uint32_t)j * (isB ? stepB : stepA));
    const uint32_t off = ok ? (isB ? voffB : voffA) : OOB;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(isB ? (nx ? rsBn : rsB) : (nx ? rsAn : rsA), IA_LDS(dst), 16, off, (int)soff, 0, 0);
  };

  // ---- the first tile's prologue: k-tiles 0 and 1 whole, landed (once per launch), first set.  Every tile's first trip then finds the
  // same state: k-tile 1 requested in full BEFORE anything else that is in flight (below).
#pragma unroll
  for (int i = 0; i < 16; ++i) dma(0, i, off_of(0), 0u);
#pragma unroll
  for (int i = 0; i < 16; ++i) dma(1, i, off_of(1), (uint32_t)(2 * TILE_BYTES));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  Op<false> a0, a1, a2, a3, b0, b1, b2, b3;
#pragma unroll
  for (int j = 0; j < 4; ++j) read_frag<0>(a0, j, baseA, 0u);
#pragma unroll
  for (int j = 0; j < 4; ++j) read_frag<0>(b0, j, baseB, 0u);
  uint32_t bo = 0;                                       // LDS byte offset of the buffer that holds the coming trip's k-tile

  f32x16 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  using Acc = std::false_type;

  const f32x4 no_bias[4][4] = {};
  while (true) {
    int bm, bn;
    coords(tile, bm, bn);
    const int m0_pre = bm * BM + wm * 128, n0_pre = bn * BN + wn * 128;
    int u = 0;
    uint32_t okA = 0u, okB = off_of(1);
    // one trip = one k-tile (t256w::main_loop, ROUND schedule, with the look-ahead reaching into the next tile)
    // A tile's FIRST trip: the last four pieces of its k-tile 1 went out in front of the previous tile's drain (or in the launch
    // prologue), so the counted wait of this trip -- "k-tile 1 has landed" -- can leave the drain's 32 output stores in flight with the 8
    // pieces it has just issued: vmcnt(40).  VMEM retires in order: with those four pieces issued BEHIND the stores (T256W's order) the
    // wait was for the stores' completion, i.e. for the whole drain of 128 KiB at the ~18 B per clock a CU's stores sustain.
    auto trip = [&](auto FIRST_T) {
      constexpr bool FIRST = decltype(FIRST_T)::value;
      const uint32_t bn_ = bo ^ (uint32_t)(2 * TILE_BYTES);
      tie2<0>(a0, b0);
      mfma_step<FIRST>(acc, a0, b0, [&](int i) {
        if (i < 4) { read_frag<1>(a1, i, baseA, bo); read_frag<1>(b1, i, baseB, bo); }
        else if (i < 8) { read_frag<2>(a2, i - 4, baseA, bo); read_frag<2>(b2, i - 4, baseB, bo); }
        else if (i < 12) { read_frag<3>(a3, i - 8, baseA, bo); read_frag<3>(b3, i - 8, baseB, bo); }
        if (!FIRST && i % 4 == 3) dma(u + 1, 12 + i / 4, okB, bn_);       // the last four pieces of k-tile u+1 (into the other buffer)
        if (i == 12) okA = off_of(u + 2);
      });
      tie6<0>(a1, b1, a2, b2, a3, b3);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      mfma_step<false>(acc, a1, b1, [&](int i) {
        if (i % 4 == 1) dma(u + 2, i / 4, okA, bo);
      });
      mfma_step<false>(acc, a2, b2, [&](int i) {
        if (i % 4 == 1) dma(u + 2, 4 + i / 4, okA, bo);
        if (i == 14) okB = off_of(u + 2);
      });
      if constexpr (FIRST) asm volatile("s_waitcnt vmcnt(40)" ::: "memory");      // 8 pieces + the previous tile's 32 stores
      else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      mfma_step<false>(acc, a3, b3, [&](int i) {
        if (i < 4) read_frag<0>(a0, i, baseA, bn_);
        else if (i < 8) read_frag<0>(b0, i - 4, baseB, bn_);
        if (i % 4 == 3) dma(u + 2, 8 + i / 4, okB, bo);
      });
      bo = bn_;
      ++u;
    };
    trip(std::true_type{});
    do { trip(Acc{}); } while (u < n_tiles);
    // the next tile's k-tile 1: its last four pieces in front of the drain's stores (see trip)
    {
      const uint32_t ok1 = off_of(n_tiles + 1), b1_ = bo ^ (uint32_t)(2 * TILE_BYTES);
#pragma unroll
      for (int i = 12; i < 16; ++i) dma(n_tiles + 1, i, ok1, b1_);
    }

    // ---- drain (t256w's plain epilogue); the pipeline stays loaded: a0 / b0 requested, k-tile 1 of the next tile in flight
    int lane_e = lane0;
    asm volatile("" : "+v"(lane_e));
    int m0 = m0_pre, n0 = n0_pre;
    asm volatile("" : "+s"(m0), "+s"(n0));
    char* stg = smem + 2 * 2 * TILE_BYTES + wave * 2 * STAGE_BYTES;
    if constexpr (SLAB) {
      const RowSlab rs = slab_rows<false>(p, bm, wm, n_live);
      drain_half_plain<false, 0, false, true, true>(p, acc, m0, n0, stg, lane_e, no_bias, 1.f, RowBlk{}, rs);
      drain_half_plain<false, 1, false, true, true>(p, acc, m0, n0 + 64, stg, lane_e, no_bias, 1.f, RowBlk{}, rs);
    } else if constexpr (ROWS) {
      const Blk8 bl = load_blk8(p.row_blk, bm, n_live);
      RowBlk rb;
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) rb.r[mi] = (wm ? bl.b[4 + mi] : bl.b[mi]) * 32;      // (-1 -> negative: none)
      drain_half_plain<false, 0, false, true>(p, acc, m0, n0, stg, lane_e, no_bias, 1.f, rb);
      drain_half_plain<false, 1, false, true>(p, acc, m0, n0 + 64, stg, lane_e, no_bias, 1.f, rb);
    } else {
    drain_half_plain<false, 0, false>(p, acc, m0, n0, stg, lane_e, no_bias);
    drain_half_plain<false, 1, false>(p, acc, m0, n0 + 64, stg, lane_e, no_bias);
    }
    tile += (int)gridDim.x;
    if (tile >= total_tiles) break;
    rsA = rsAn; rsB = rsBn;
    rsAn = window_a(tile + (int)gridDim.x); rsBn = window_b(tile + (int)gridDim.x);
    if constexpr (ROWS) { roA = roAn; roAn = rows_a(tile + (int)gridDim.x); }
  }
  tie2<0>(a0, b0);                                        // dead, but in flight
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the look-ahead pieces of the tile that does not exist target this workgroup's LDS
