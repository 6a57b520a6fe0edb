// kma_kmersets.h — the ProteinKmers sets of a batch and the postings of their keys
// (kma_kmersets.hip): launchers used by kma_abi_sets.cpp, and the small device helpers the set
// operators' units share (kma_kmersets.hip, kma_distance.hip, kma_hashanno.hip,
// kma_hashindex.hip). Not part of the public ABI (see include/kmeranno.h).
//
// ProteinKmers (external org.theseed.sequence, restated): the SET of distinct length-K substrings
// of a protein at i = 0 .. L-K. On the device, for batches of proteins and any protein length:
//   window_keys_kernel  every window of every protein packed to a 5K-bit key (K <= 12) at its
//                       residue position; positions that start no window hold the sentinel
//   (rocPRIM) segmented radix sort of each protein's positions
//   distinct_kernel     |S| per protein: first occurrences of non-sentinel keys (wave per protein)
//   owner_first_kernel  per position: its protein, and whether it is such a first occurrence
// and the postings of those sets: the (key, owner) pairs of the first occurrences (two selects)
// sorted by key with the stable radix sort, so that a key's owners ascend; run_heads_kernel
// marks the first pair of every key, two more selects leave the unique keys and their range
// starts, and set_end_kernel closes the last range.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kma {

// The key of a position that starts no window: above every 5K-bit key, so last in sort order.
constexpr uint64_t kKeySentinel = ~0ull;

// Position p of the sorted segment that starts at lo holds the first occurrence of a key of the
// set (v = sorted[p], which the caller has loaded).
__device__ __forceinline__ bool set_head(uint64_t v, const uint64_t* __restrict__ sorted,
                                         uint64_t lo, uint64_t p) {
  return v != kKeySentinel && (p == lo || sorted[p - 1] != v);
}

// First index in [lo, hi) of the ascending keys a with a[index] >= v (hi if none).
__device__ __forceinline__ uint64_t lower_bound(const uint64_t* __restrict__ a, uint64_t lo,
                                                uint64_t hi, uint64_t v) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Sum of v over the wave's 64 lanes, in every lane.
__device__ __forceinline__ uint32_t dwave_sum(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// Blocks for n items at per_block items a block: at least one, at most cap (the kernels stride).
inline unsigned grid_blocks(uint64_t n, unsigned per_block, unsigned cap) {
  const uint64_t g = (n + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}
inline unsigned grid1(uint64_t n) { return grid_blocks(n, 256, 8192); }        // thread per item
inline unsigned grid_waves(uint64_t n) { return grid_blocks(n, 4, 16384); }    // wave per item

// keys[p] of every residue position p (relative to off[0]); a window starts at i < L - K + 1
// (L - K with end_exclusive). A byte outside A-Z / '*' in a window raises *alpha.
hipError_t launch_window_keys(const uint8_t* res, const uint64_t* off, uint32_t n, int k,
                              int end_exclusive, uint64_t* keys, uint32_t* alpha, hipStream_t s);
hipError_t launch_segmented_sort(void* temp, size_t* temp_bytes, const uint64_t* in,
                                 uint64_t* out, uint64_t n_items, uint32_t n_seg,
                                 const uint64_t* seg_begin, const uint64_t* seg_end, int bits,
                                 hipStream_t s);
hipError_t launch_distinct(const uint64_t* sorted, const uint64_t* off, uint32_t n, uint32_t* size,
                           hipStream_t s);
hipError_t launch_owner_first(const uint64_t* sorted, const uint64_t* off, uint32_t n,
                              uint32_t* owner, uint8_t* first, hipStream_t s);
// head[i] = 1 where k[i] starts a run of equal keys; idx[i] = i.
hipError_t launch_run_heads(const uint64_t* k, uint64_t n, uint8_t* head, uint32_t* idx,
                            hipStream_t s);
// ustart[*n_u] = n_pairs.
hipError_t launch_set_end(uint32_t* ustart, const uint64_t* n_u, uint64_t n_pairs, hipStream_t s);
// rocPRIM wrappers (temp == nullptr: size query).
hipError_t prim_select_flagged_u64(void* temp, size_t* tb, const uint64_t* in, const uint8_t* f,
                                  uint64_t* out, uint64_t* n_out, uint64_t n, hipStream_t s);
hipError_t prim_select_flagged_u32(void* temp, size_t* tb, const uint32_t* in, const uint8_t* f,
                                  uint32_t* out, uint64_t* n_out, uint64_t n, hipStream_t s);
hipError_t prim_sort_pairs_u64_u32(void* temp, size_t* tb, const uint64_t* ki, uint64_t* ko,
                                  const uint32_t* vi, uint32_t* vo, uint64_t n, int bits,
                                  hipStream_t s);

}  // namespace kma
