// kma_kmersets.hip — the ProteinKmers sets of a batch and the postings of their keys on the
// device (kma_kmersets.h has the GPU form): the one home of these kernels for
// kma_protein_distances, kma_hash_annotate, kma_proto_index_create and
// kma_hash_annotate_indexed (kma_abi_sets.cpp).
#include <cstring>  // (rocprim.hpp uses memset without including it)
#include <rocprim/rocprim.hpp>

#include "kma_kmersets.h"

namespace kma {
namespace {

// Wave per protein: keys[p] for every residue position p of protein s (relative to off[0]);
// a window starts at i < n_win(s) = L - K + 1 (or L - K with end_exclusive). A byte outside
// A-Z / '*' in a window raises *alpha (the caller refuses the batch).
__global__ __launch_bounds__(256) void window_keys_kernel(const uint8_t* __restrict__ res,
                                                          const uint64_t* __restrict__ off,
                                                          uint32_t n, int k, int end_exclusive,
                                                          uint64_t* __restrict__ keys,
                                                          uint32_t* __restrict__ alpha) {
  __shared__ uint8_t lut[256];
  const int t = threadIdx.x;
  lut[t] = (t >= 'A' && t <= 'Z') ? (uint8_t)(t - 'A' + 1) : (t == '*' ? 27 : 0);
  __syncthreads();
  const uint32_t lane = t & 63;
  const uint64_t o0 = off[0];
  for (uint64_t s = (uint64_t)blockIdx.x * 4 + (t >> 6); s < n; s += (uint64_t)gridDim.x * 4) {
    const uint64_t lo = off[s], hi = off[s + 1];
    const int64_t n_win = (int64_t)(hi - lo) - k + (end_exclusive ? 0 : 1);
    bool bad = false;
    for (uint64_t p = lo + lane; p < hi; p += 64) {
      const int64_t i = (int64_t)(p - lo);
      uint64_t key = kKeySentinel;
      if (i < n_win) {
        uint64_t v = 0;
        bool ok = true;
        for (int j = 0; j < k; ++j) {
          const uint32_t c = lut[res[p + j]];
          ok = ok && c != 0u;
          v = (v << 5) | c;
        }
        bad = bad || !ok;
        key = v;
      }
      keys[p - o0] = key;
    }
    if (__ballot(bad) && lane == 0) atomicOr(alpha, 1u);
  }
}

// Wave per protein: distinct non-sentinel keys of its sorted segment.
__global__ __launch_bounds__(256) void distinct_kernel(const uint64_t* __restrict__ sorted,
                                                       const uint64_t* __restrict__ off,
                                                       uint32_t n, uint32_t* __restrict__ size) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t o0 = off[0];
  for (uint64_t s = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < n;
       s += (uint64_t)gridDim.x * 4) {
    const uint64_t lo = off[s] - o0, hi = off[s + 1] - o0;
    uint32_t c = 0;
    for (uint64_t p = lo + lane; p < hi; p += 64) {
      const uint64_t v = sorted[p];
      c += set_head(v, sorted, lo, p) ? 1u : 0u;
    }
    c = dwave_sum(c);
    if (lane == 0) size[s] = c;
  }
}

// Wave per protein: owner[p] = protein of position p; first[p] = 1 at the first occurrence of a
// non-sentinel key in the protein's sorted segment.
__global__ __launch_bounds__(256) void owner_first_kernel(const uint64_t* __restrict__ sorted,
                                                          const uint64_t* __restrict__ off,
                                                          uint32_t n, uint32_t* __restrict__ owner,
                                                          uint8_t* __restrict__ first) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t o0 = off[0];
  for (uint64_t s = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < n;
       s += (uint64_t)gridDim.x * 4) {
    const uint64_t lo = off[s] - o0, hi = off[s + 1] - o0;
    for (uint64_t p = lo + lane; p < hi; p += 64) {
      const uint64_t v = sorted[p];
      owner[p] = (uint32_t)s;
      first[p] = set_head(v, sorted, lo, p) ? 1 : 0;
    }
  }
}

__global__ __launch_bounds__(256) void run_heads_kernel(const uint64_t* __restrict__ k,
                                                        uint64_t n, uint8_t* __restrict__ head,
                                                        uint32_t* __restrict__ idx) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) {
    head[i] = (i == 0 || k[i] != k[i - 1]) ? 1 : 0;
    idx[i] = (uint32_t)i;
  }
}

__global__ void set_end_kernel(uint32_t* ustart, const uint64_t* n_u, uint64_t n_pairs) {
  ustart[*n_u] = (uint32_t)n_pairs;
}

}  // namespace

hipError_t launch_window_keys(const uint8_t* res, const uint64_t* off, uint32_t n, int k,
                              int end_exclusive, uint64_t* keys, uint32_t* alpha,
                              hipStream_t s) {
  hipLaunchKernelGGL(window_keys_kernel, dim3(grid_waves(n)), dim3(256), 0, s, res, off, n, k,
                     end_exclusive, keys, alpha);
  return hipGetLastError();
}

hipError_t launch_segmented_sort(void* temp, size_t* temp_bytes, const uint64_t* in,
                                 uint64_t* out, uint64_t n_items, uint32_t n_seg,
                                 const uint64_t* seg_begin, const uint64_t* seg_end, int bits,
                                 hipStream_t s) {
  return rocprim::segmented_radix_sort_keys(temp, *temp_bytes, in, out, (unsigned)n_items, n_seg,
                                            seg_begin, seg_end, 0u, (unsigned)bits, s);
}

hipError_t launch_distinct(const uint64_t* sorted, const uint64_t* off, uint32_t n, uint32_t* size,
                           hipStream_t s) {
  hipLaunchKernelGGL(distinct_kernel, dim3(grid_waves(n)), dim3(256), 0, s, sorted, off, n, size);
  return hipGetLastError();
}

hipError_t launch_owner_first(const uint64_t* sorted, const uint64_t* off, uint32_t n,
                              uint32_t* owner, uint8_t* first, hipStream_t s) {
  hipLaunchKernelGGL(owner_first_kernel, dim3(grid_waves(n)), dim3(256), 0, s, sorted, off, n,
                     owner, first);
  return hipGetLastError();
}
hipError_t launch_run_heads(const uint64_t* k, uint64_t n, uint8_t* head, uint32_t* idx,
                            hipStream_t s) {
  hipLaunchKernelGGL(run_heads_kernel, dim3(grid1(n)), dim3(256), 0, s, k, n, head, idx);
  return hipGetLastError();
}
hipError_t launch_set_end(uint32_t* ustart, const uint64_t* n_u, uint64_t n_pairs, hipStream_t s) {
  hipLaunchKernelGGL(set_end_kernel, dim3(1), dim3(1), 0, s, ustart, n_u, n_pairs);
  return hipGetLastError();
}

// rocPRIM wrappers (temp == nullptr: size query).
hipError_t prim_select_flagged_u64(void* temp, size_t* tb, const uint64_t* in, const uint8_t* f,
                                  uint64_t* out, uint64_t* n_out, uint64_t n, hipStream_t s) {
  return rocprim::select(temp, *tb, in, f, out, n_out, (size_t)n, s);
}
hipError_t prim_select_flagged_u32(void* temp, size_t* tb, const uint32_t* in, const uint8_t* f,
                                  uint32_t* out, uint64_t* n_out, uint64_t n, hipStream_t s) {
  return rocprim::select(temp, *tb, in, f, out, n_out, (size_t)n, s);
}
hipError_t prim_sort_pairs_u64_u32(void* temp, size_t* tb, const uint64_t* ki, uint64_t* ko,
                                  const uint32_t* vi, uint32_t* vo, uint64_t n, int bits,
                                  hipStream_t s) {
  return rocprim::radix_sort_pairs(temp, *tb, ki, ko, vi, vo, (size_t)n, 0u, (unsigned)bits, s);
}

}  // namespace kma
