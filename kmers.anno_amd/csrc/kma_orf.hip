// kma_orf.hip — ORF extension of the projector's peg proposals on the device.
//
// PegProposalList.propose (locations/PegProposalList.java:67-77) begins with PegProposal.create
// -> Location.extend(genome) (locations/PegProposal.java:50-58): the proposal grows to the whole
// ORF around it, its right end to the next in-frame stop, its left end to the farthest start
// codon since the previous in-frame stop. Walked codon by codon that is hundreds of steps per
// proposal; here both answers are read from two arrays that depend on the genome alone and are
// built once per new genome (up to 10 close genomes are projected onto it,
// anno/KmerProcessor.java:185):
//
//   orf_classify_kernel  one pass over the contig bytes: per (contig, strand, frame, codon) slot
//                        the operands of the two scans; the '-' strand from the same bytes in
//                        registers (no reverse-complement copy), frame-major so that a frame is
//                        a contiguous segment (layout: kma_orf.h)
//   inclusive_scan x 2   rocPRIM, in place, OrfScanOp: stop_at backwards (reverse iterators),
//                        start_at forwards
//   orf_extend_kernel    one thread per proposal: two loads, the strand mapping, the three
//                        filters; counters by one atomic per wave
//
// O(bases) per index, O(1) per proposal: no thread walks codons. Location.extend is external to
// the reference; its restated semantics (include/kmeranno.h) are parity-unpinned.
#include <cstring>  // (rocprim.hpp uses memset without including it)
#include <rocprim/rocprim.hpp>

#include "../../include/kmeranno.h"
#include "kma_orf.h"

namespace kma {
namespace {

__global__ __launch_bounds__(256) void orf_classify_kernel(OrfBuildArgs a) {
  for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < a.half;
       t += (uint64_t)gridDim.x * 256u)
    orf_classify(a, t);
}

__device__ __forceinline__ void count_wave(uint64_t* stat, bool pred) {
  const uint64_t m = __ballot(pred);
  if (m && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(m))
    atomicAdd((unsigned long long*)stat, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(256) void orf_extend_kernel(OrfExtendArgs a) {
  const uint64_t n_iter = (a.n + 255u) / 256u * 256u;  // every lane reaches the ballots
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_iter;
       i += (uint64_t)gridDim.x * 256u) {
    const bool live = i < a.n;
    uint32_t st = KMA_ORF_KEPT;
    if (live) {
      int32_t l, r;
      st = orf_extend(a, a.props[i], &l, &r);
      a.left[i] = l;
      a.right[i] = r;
      a.status[i] = (uint8_t)st;
    }
    count_wave(a.stats + 0, live);
    count_wave(a.stats + 1, live && st == KMA_ORF_REJECTED);
    count_wave(a.stats + 2, live && st == KMA_ORF_WEAK);
    count_wave(a.stats + 3, live && st == KMA_ORF_SMALL);
  }
}

unsigned grid_of(uint64_t n) {
  const uint64_t g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace

hipError_t launch_orf_build(const OrfBuildArgs& a, void* temp, size_t* temp_bytes,
                            hipStream_t stream) {
  const size_t slots = 2 * (size_t)a.half;
  const OrfScanOp op;
  const auto stop_rev = rocprim::make_reverse_iterator(a.stop_at + slots);
  if (!temp) {
    size_t s1 = 0, s2 = 0;
    hipError_t e = rocprim::inclusive_scan(nullptr, s1, a.start_at, a.start_at, slots, op, stream);
    if (e != hipSuccess) return e;
    e = rocprim::inclusive_scan(nullptr, s2, stop_rev, stop_rev, slots, op, stream);
    if (e != hipSuccess) return e;
    *temp_bytes = std::max(s1, s2);
    return hipSuccess;
  }
  if (slots == 0) return hipSuccess;
  hipLaunchKernelGGL(orf_classify_kernel, dim3(grid_of(a.half)), dim3(256), 0, stream, a);
  size_t tb = *temp_bytes;
  hipError_t e = rocprim::inclusive_scan(temp, tb, a.start_at, a.start_at, slots, op, stream);
  if (e != hipSuccess) return e;
  tb = *temp_bytes;
  e = rocprim::inclusive_scan(temp, tb, stop_rev, stop_rev, slots, op, stream);
  if (e != hipSuccess) return e;
  return hipGetLastError();
}

hipError_t launch_orf_extend(const OrfExtendArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(orf_extend_kernel, dim3(grid_of(a.n)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace kma
