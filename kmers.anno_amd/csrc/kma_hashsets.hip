// kma_hashsets.hip — the genome side of the indexed hash annotator for a device-resident batch
// (§8(f)3; kma_hashsets.h has the pieces shared with the host check program).
//
// genome_sets_kernel: one 256-thread workgroup per genome protein, on a grid-stride over the
// proteins as index_score_kernel has it. It stands, for kma_hash_annotate_indexed_device, where
// the host entry runs window_keys_kernel, the segmented sort, distinct_kernel,
// owner_first_kernel and index_lookup_kernel:
//   codes    the chunk's residues (its windows' bytes and no others) through the 256-entry LUT
//            into LDS; a code of 0 is a byte outside the alphabet inside a window
//   keys     one 5K-bit key per window from the LDS codes, the rest of the network's size padded
//            with kKeySentinel
//   sort     bitonic network in LDS over the next power of two at or above the chunk's windows.
//            A wave's 64 compare-exchanges of a step cover one aligned tile of 128 keys, and
//            every stride of 64 or less stays inside that tile: those steps run back to back in
//            the wave (its LDS operations complete in order), and only the wider strides and
//            the end of every merge width meet at a workgroup barrier
//   heads    a key that differs from its predecessor and, in a protein of several chunks, lies
//            in no earlier run of the protein (the runs are in the scratch's key area, written
//            by this block and read after a barrier); a head is looked up in the index's unique
//            keys and its match goes to gmatch at the key's sorted position
// Which position carries which head does not matter to index_score_kernel, which sums over the
// protein's segment of gmatch; duplicates, misses and the K - 1 trailing positions hold
// kHashEmpty, so every position of every protein is written.
//
// LDS: 32 KB of keys, 4 KB of codes, the LUT: four workgroups per CU. An 8-byte compare-exchange
// of stride 32 or more reads 32 consecutive keys per lane group (conflict-free); below that a
// lane group spans 64 keys and every other one, two per bank pair (2-way).
#include "kma_hashsets.h"

#include "kma_hashindex.h"
#include "kma_kmersets.h"

namespace kma {
namespace {

__device__ __forceinline__ void compare_exchange(uint64_t* key, uint32_t t, uint32_t j,
                                                 uint32_t m) {
  const uint32_t lo = sets_step_low(t, j), hi = lo | j;
  const uint64_t x = key[lo], y = key[hi];
  if ((x > y) == sets_step_ascending(lo, m)) {
    key[lo] = y;
    key[hi] = x;
  }
}

// The wave's earlier LDS writes before its later LDS reads (other lanes' keys of the same tile).
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// key[0 .. n2) ascending (n2 a power of two; block-uniform arguments; ends on a barrier).
__device__ __forceinline__ void block_bitonic_sort(uint64_t* key, uint32_t n2, uint32_t tid) {
  const uint32_t half = n2 >> 1;
  for (uint32_t m = 2; m <= n2; m <<= 1) {
    uint32_t j = m >> 1;
    for (; j > 64; j >>= 1) {
      for (uint32_t t = tid; t < half; t += kSetsBlock) compare_exchange(key, t, j, m);
      __syncthreads();
    }
    for (uint32_t t = tid; t < half; t += kSetsBlock)
      for (uint32_t jj = j; jj; jj >>= 1) {
        compare_exchange(key, t, jj, m);
        wave_lds_fence();
      }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void genome_sets_kernel(GenomeSetsArgs a) {
  __shared__ uint64_t s_key[kSetsKeysMax];
  __shared__ uint8_t s_code[kSetsKeysMax + kSetsCodePad];
  __shared__ uint8_t s_lut[256];
  __shared__ uint32_t s_heads;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t W = a.w, k = (uint32_t)a.k;
  s_lut[tid] = (uint8_t)sets_code(tid);
  bool bad = false;
  const uint64_t o0 = a.off[0];
  for (uint32_t g = blockIdx.x; g < a.n_genome; g += gridDim.x) {
    const uint64_t lo = a.off[g], len = a.off[g + 1] - lo, seg = lo - o0;
    const uint64_t n_win = sets_windows(len, a.k);
    const bool runs_kept = n_win > W;
    uint64_t* runs = a.runs + seg;
    uint32_t heads = 0;
    __syncthreads();  // (the LUT; the protein before: its last read of s_heads)
    if (tid == 0) s_heads = 0;
    uint32_t c = 0;
    for (uint64_t c0 = 0; c0 < n_win; c0 += W, ++c) {
      const uint32_t nw = (uint32_t)(n_win - c0 < W ? n_win - c0 : W);
      const uint32_t n2 = sets_padded_size(nw);
      __syncthreads();  // (the chunk before: its reads of s_key, its writes of its run)
      for (uint32_t i = tid; i < nw + k - 1; i += kSetsBlock) {
        const uint32_t code = s_lut[a.res[lo + c0 + i]];
        bad = bad || code == 0u;
        s_code[i] = (uint8_t)code;
      }
      __syncthreads();
      for (uint32_t i = tid; i < n2; i += kSetsBlock)
        s_key[i] = i < nw ? sets_window_key(s_code + i, a.k) : kKeySentinel;
      __syncthreads();
      block_bitonic_sort(s_key, n2, tid);
      for (uint32_t j = tid; j < nw; j += kSetsBlock) {
        const uint64_t v = s_key[j];
        uint32_t match = kHashEmpty;
        if (sets_is_head(s_key, j, runs, c, W)) {
          ++heads;
          const uint64_t at = lower_bound(a.ukeys, 0, a.n_u, v);
          if (at < a.n_u && a.ukeys[at] == v) match = (uint32_t)at;
        }
        a.gmatch[seg + c0 + j] = match;
        if (runs_kept) runs[c0 + j] = v;
      }
    }
    for (uint64_t p = n_win + tid; p < len; p += kSetsBlock) a.gmatch[seg + p] = kHashEmpty;
    heads = dwave_sum(heads);
    if (lane == 0 && heads) atomicAdd(&s_heads, heads);
    __syncthreads();
    if (tid == 0) a.gsize[g] = s_heads;
  }
  if (bad) atomicOr(a.alpha, 1ull);
}

// The outputs' start values, in a kernel of the call's chain: count and stats to zero and,
// for an index of no prototypes (n_default > 0), every protein's default proposal.
__global__ __launch_bounds__(256) void hash_reset_kernel(uint32_t* count, uint32_t n_count,
                                                         unsigned long long* stats,
                                                         int32_t* best, double* sim,
                                                         uint32_t n_default) {
  const uint64_t i0 = blockIdx.x * 256ull + threadIdx.x, step = gridDim.x * 256ull;
  for (uint64_t i = i0; i < n_count; i += step) count[i] = 0;
  for (uint64_t i = i0; i < n_default; i += step) best[i] = -1, sim[i] = 0.0;
  if (i0 < 4) stats[i0] = 0;
}

}  // namespace

hipError_t launch_hash_reset(uint32_t* count, uint32_t n_count, unsigned long long* stats,
                             int32_t* best, double* sim, uint32_t n_default, hipStream_t s) {
  const uint32_t n = n_count > n_default ? n_count : n_default;
  hipLaunchKernelGGL(hash_reset_kernel, dim3(grid1(n)), dim3(256), 0, s, count, n_count, stats,
                     best, sim, n_default);
  return hipGetLastError();
}

hipError_t launch_genome_sets(const GenomeSetsArgs& a, hipStream_t s) {
  if (a.n_genome == 0 || a.k < 2 || a.k > 12 || a.w < kSetsKeysMin || a.w > kSetsKeysMax ||
      (a.w & (a.w - 1u)))
    return hipErrorInvalidValue;
  const unsigned grid = a.n_genome > (1u << 20) ? (1u << 20) : a.n_genome;
  hipLaunchKernelGGL(genome_sets_kernel, dim3(grid), dim3(kSetsBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace kma
