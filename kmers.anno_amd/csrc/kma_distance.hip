// kma_distance.hip — ProteinKmers.distance on the GPU.
//
// GeneCopyProcessor.runCommand (genome/compare/GeneCopyProcessor.java:129-162) compares every
// target peg's ProteinKmers with those of the source pegs of the same function and keeps the
// closest one within maxDist. ProteinKmers (external org.theseed.sequence, restated): the SET
// of distinct length-K substrings at i = 0 .. L-K; distance = 1 - |A n B| / |A u B| (Jaccard),
// 1.0 when the sets share nothing.
//
// GPU form: the ProteinKmers sets of the batch (kma_kmersets.hip: window keys, per-protein
// segmented sort, distinct sizes), then
//   pair_kernel         per (a, b) pair: the distinct keys of the smaller set, each looked up by
//                       binary search in the other's sorted keys (wave per pair, lanes stride)
// Integer work only; outputs are (|A|, |B|, |A n B|) per pair, the host forms the distance in
// double exactly as the restated Java expression.
#include "kma_distance.h"
#include "kma_kmersets.h"

namespace kma {
namespace {

// Wave per pair: |A n B| by looking up the distinct keys of the smaller set in the larger.
__global__ __launch_bounds__(256) void pair_kernel(const uint64_t* __restrict__ sa,
                                                   const uint64_t* __restrict__ offa,
                                                   const uint32_t* __restrict__ size_a,
                                                   const uint64_t* __restrict__ sb,
                                                   const uint64_t* __restrict__ offb,
                                                   const uint32_t* __restrict__ size_b,
                                                   const uint32_t* __restrict__ pa,
                                                   const uint32_t* __restrict__ pb,
                                                   uint64_t n_pairs, uint32_t* __restrict__ sim) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t a0 = offa[0], b0 = offb[0];
  for (uint64_t q = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < n_pairs;
       q += (uint64_t)gridDim.x * 4) {
    const uint32_t ia = pa[q], ib = pb[q];
    // segments; distinct keys come first in sort order, sentinels last
    const uint64_t* s1 = sa;
    uint64_t lo1 = offa[ia] - a0, hi1 = offa[ia + 1] - a0;
    const uint64_t* s2 = sb;
    uint64_t lo2 = offb[ib] - b0, hi2 = offb[ib + 1] - b0;
    if (size_a[ia] > size_b[ib]) {  // scan the smaller set
      const uint64_t* ts = s1; s1 = s2; s2 = ts;
      uint64_t t0 = lo1; lo1 = lo2; lo2 = t0;
      t0 = hi1; hi1 = hi2; hi2 = t0;
    }
    uint32_t c = 0;
    for (uint64_t p = lo1 + lane; p < hi1; p += 64) {
      const uint64_t v = s1[p];
      // (not a first occurrence; !set_head(v, s1, lo1, p) compiles to other compares)
      if (v == kKeySentinel || (p > lo1 && s1[p - 1] == v)) continue;
      const uint64_t j = lower_bound(s2, lo2, hi2, v);
      c += (j < hi2 && s2[j] == v) ? 1u : 0u;
    }
    c = dwave_sum(c);
    if (lane == 0) sim[q] = c;
  }
}

}  // namespace

hipError_t launch_pairs(const uint64_t* sa, const uint64_t* offa, const uint32_t* size_a,
                        const uint64_t* sb, const uint64_t* offb, const uint32_t* size_b,
                        const uint32_t* pa, const uint32_t* pb, uint64_t n_pairs, uint32_t* sim,
                        hipStream_t s) {
  hipLaunchKernelGGL(pair_kernel, dim3(grid_waves(n_pairs)), dim3(256), 0, s, sa, offa, size_a,
                     sb, offb, size_b, pa, pb, n_pairs, sim);
  return hipGetLastError();
}

}  // namespace kma
