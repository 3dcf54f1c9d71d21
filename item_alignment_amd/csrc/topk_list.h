// The sorted k-list of the streaming top-k scans (kgtopk.hip: translation distances on the vector ALU; simtopk.hip: bf16 MFMA
// similarities).  A list entry is one 64-bit key, (order word) << 32 | candidate id, chosen by the scan so that the unsigned order of
// the keys is its total order (best first, id ascending among equals).  Keys are unique, so the k smallest keys of a candidate set do
// not depend on the order in which the candidates arrive.  A list sits one entry per lane of the wave that owns it; an insertion is
// done by the whole wave.
#pragma once
#include "common.h"

namespace {

typedef unsigned long long tk_key;
constexpr tk_key TK_EMPTY = ~0ull;          // an unused slot; larger than every key (ids are < 2^31)

IA_DEV tk_key tk_lane(tk_key v, int lane) {   // lane: wave-uniform
  const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, lane), hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((tk_key)hi << 32) | lo;
}
IA_DEV tk_key tk_up1(tk_key v) {              // the value of lane - 1 (lane 0: its own)
  const uint32_t lo = __shfl_up((int)(uint32_t)v, 1), hi = __shfl_up((int)(uint32_t)(v >> 32), 1);
  return ((tk_key)hi << 32) | lo;
}
// Insert key into the sorted k-list held one entry per lane (lanes >= k hold TK_EMPTY); whole wave, key wave-uniform.
// Returns false (list unchanged) when key is not among the k smallest.
IA_DEV bool tk_insert(tk_key& e, tk_key key, int k, int lane, int& pos) {
  pos = __popcll(__ballot(e < key));
  if (pos >= k) return false;
  const tk_key prev = tk_up1(e);
  e = lane < pos ? e : (lane == pos ? key : prev);
  if (lane >= k) e = TK_EMPTY;
  return true;
}
// The merge of the splits, one wave per query: part[(b * n_splits + s) * k + l] is the (sorted) list of query b over split s; every
// split's list is inserted entry by entry until one fails.  Returns the merged list, entry `lane` in lane `lane`.
IA_DEV tk_key tk_merge(const tk_key* __restrict__ part, int b, int k, int n_splits, int lane) {
  tk_key cur = TK_EMPTY;
  for (int s = 0; s < n_splits; ++s) {
    const tk_key mine = lane < k ? part[((size_t)b * n_splits + s) * k + lane] : TK_EMPTY;
    for (int t = 0; t < k; ++t) {
      const tk_key key = tk_lane(mine, t);
      int pos;
      if (key == TK_EMPTY || !tk_insert(cur, key, k, lane, pos)) break;
    }
  }
  return cur;
}

}  // namespace
