// kma_hashanno.hip — the hash annotator's scoring loop on the device (§8(f)3).
//
// HashAnnotationProcessor.processGenome (HashAnnotationProcessor.java:221-328): a genome's
// proteins go into a GenomeProteinKmers index (:233-248), every prototype of the role
// annotation file is scored against it in file order (processProposal, :259-271), and each
// protein keeps its best proposal (getProposal, :278-306). GenomeProteinKmers is external
// (org.theseed.proteins.kmers, not in the reference); restated as in oracle/kma_oracle.c
// orc_hash_annotate: distinct K-mer sets (ProteinKmers, windows i = 0 .. L-K), similarity =
// shared / (|A| + |B| - shared), a prototype becomes a protein's proposal when its similarity
// is >= minSim and above the current one (earlier prototypes win ties).
//
// GPU form (sorts and scans; no per-pair loop):
//   genome:     its ProteinKmers sets and their postings (kma_kmersets.hip): (key, protein) pairs
//               of distinct keys sorted by key, unique keys U with their protein ranges
//   prototypes: their ProteinKmers sets (kma_kmersets.hip); every distinct key looked up in U
//               (binary search) and one candidate (prototype, protein) emitted per protein of
//               its range; candidates sorted and run-length encoded: the run length IS the
//               number of shared distinct kmers
//   score:      similarity per (prototype, protein) in double (the Java expression), match
//               counts per prototype, best similarity per protein (u64 atomicMax on the
//               non-negative double's bits), then the smallest prototype index at that value
#include <cstring>  // (rocprim.hpp uses memset without including it)
#include <rocprim/rocprim.hpp>

#include "kma_hashanno.h"
#include "kma_kmersets.h"

namespace kma {
namespace {

// The u with U[u] == v, or n if there is none.
__device__ __forceinline__ uint64_t find_key(const uint64_t* __restrict__ U, uint64_t n,
                                             uint64_t v) {
  const uint64_t lo = lower_bound(U, 0, n, v);
  return (lo < n && U[lo] == v) ? lo : n;
}

// Per prototype position: the genome proteins sharing its key (first occurrences only).
__global__ __launch_bounds__(256) void cand_count_kernel(HashArgs a) {
  const uint64_t n_u = *a.n_u;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < a.n_ppos; i += gridDim.x * 256ull) {
    uint32_t c = 0, u = 0;
    if (a.pfirst[i]) {
      const uint64_t f = find_key(a.ukeys, n_u, a.psorted[i]);
      if (f < n_u) {
        u = (uint32_t)f;
        c = a.ustart[f + 1] - a.ustart[f];
      }
    }
    a.ccount[i] = c;
    a.cu[i] = u;
  }
}

// The slice's candidates: positions [pos_lo, pos_hi), written from cand_base.
__global__ __launch_bounds__(256) void cand_emit_kernel(HashArgs a) {
  for (uint64_t i = a.pos_lo + blockIdx.x * 256ull + threadIdx.x; i < a.pos_hi;
       i += gridDim.x * 256ull) {
    const uint32_t c = a.ccount[i];
    if (!c) continue;
    const uint64_t o = a.coff[i] - a.cand_base, proto = a.powner[i];
    const uint32_t s = a.ustart[a.cu[i]];
    for (uint32_t j = 0; j < c; ++j) a.cand[o + j] = proto << 32 | a.gprot[s + j];
  }
}

__device__ __forceinline__ double sim_of(const HashArgs& a, uint64_t pair, uint32_t c,
                                         uint32_t& proto, uint32_t& gp) {
  proto = (uint32_t)(pair >> 32);
  gp = (uint32_t)pair;
  const double uni = (double)a.psize[proto] + (double)a.gsize[gp] - (double)c;
  return (double)c / uni;
}

__global__ __launch_bounds__(256) void score_kernel(HashArgs a) {
  const uint64_t n = *a.n_runs;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) {
    uint32_t proto, gp;
    const double s = sim_of(a, a.runs[i], a.run_len[i], proto, gp);
    if (s >= a.min_sim) {
      atomicAdd(a.out_count + proto, 1u);
      atomicMax((unsigned long long*)(a.best_bits + gp),
                (unsigned long long)__double_as_longlong(s));
    }
  }
}

__global__ __launch_bounds__(256) void choose_kernel(HashArgs a) {
  const uint64_t n = *a.n_runs;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) {
    uint32_t proto, gp;
    const double s = sim_of(a, a.runs[i], a.run_len[i], proto, gp);
    if (s >= a.min_sim && (uint64_t)__double_as_longlong(s) == a.best_bits[gp])
      atomicMin(a.best_proto + gp, proto);
  }
}

__global__ __launch_bounds__(256) void proto_cum_kernel(const uint64_t* __restrict__ coff,
                                                        const uint32_t* __restrict__ ccount,
                                                        const uint64_t* __restrict__ off,
                                                        uint32_t n_proto, uint64_t n_pos,
                                                        uint64_t* __restrict__ cum) {
  const uint64_t total = n_pos ? coff[n_pos - 1] + ccount[n_pos - 1] : 0;
  const uint64_t o0 = off[0];
  for (uint64_t p = blockIdx.x * 256ull + threadIdx.x; p <= n_proto; p += gridDim.x * 256ull) {
    const uint64_t pos = off[p] - o0;
    cum[p] = pos < n_pos ? coff[pos] : total;
  }
}

__global__ __launch_bounds__(256) void merge_best_kernel(uint64_t* __restrict__ best_bits,
                                                         uint32_t* __restrict__ best_proto,
                                                         uint64_t* __restrict__ slice_bits,
                                                         uint32_t* __restrict__ slice_proto,
                                                         uint32_t n) {
  for (uint64_t g = blockIdx.x * 256ull + threadIdx.x; g < n; g += gridDim.x * 256ull) {
    const uint32_t sp = slice_proto[g];
    if (sp != 0xFFFFFFFFu && (best_proto[g] == 0xFFFFFFFFu || slice_bits[g] > best_bits[g])) {
      best_bits[g] = slice_bits[g];
      best_proto[g] = sp;
    }
    slice_bits[g] = 0;
    slice_proto[g] = 0xFFFFFFFFu;
  }
}

}  // namespace

hipError_t launch_proto_cum(const uint64_t* coff, const uint32_t* ccount, const uint64_t* off,
                            uint32_t n_proto, uint64_t n_pos, uint64_t* cum, hipStream_t s) {
  hipLaunchKernelGGL(proto_cum_kernel, dim3(grid1((uint64_t)n_proto + 1)), dim3(256), 0, s, coff,
                     ccount, off, n_proto, n_pos, cum);
  return hipGetLastError();
}
hipError_t launch_merge_best(uint64_t* best_bits, uint32_t* best_proto, uint64_t* slice_bits,
                             uint32_t* slice_proto, uint32_t n, hipStream_t s) {
  hipLaunchKernelGGL(merge_best_kernel, dim3(grid1(n)), dim3(256), 0, s, best_bits, best_proto,
                     slice_bits, slice_proto, n);
  return hipGetLastError();
}

hipError_t launch_cand_count(const HashArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(cand_count_kernel, dim3(grid1(a.n_ppos)), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_cand_emit(const HashArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(cand_emit_kernel, dim3(grid1(a.pos_hi - a.pos_lo)), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_score(const HashArgs& a, uint64_t n_max, hipStream_t s) {
  hipLaunchKernelGGL(score_kernel, dim3(grid1(n_max)), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_choose(const HashArgs& a, uint64_t n_max, hipStream_t s) {
  hipLaunchKernelGGL(choose_kernel, dim3(grid1(n_max)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// rocPRIM wrappers (temp == nullptr: size query).
hipError_t prim_sort_keys_u64(void* temp, size_t* tb, const uint64_t* ki, uint64_t* ko, uint64_t n,
                             int bits, hipStream_t s) {
  return rocprim::radix_sort_keys(temp, *tb, ki, ko, (size_t)n, 0u, (unsigned)bits, s);
}
hipError_t prim_excl_sum_u32_u64(void* temp, size_t* tb, const uint32_t* in, uint64_t* out,
                                uint64_t n, hipStream_t s) {
  return rocprim::exclusive_scan(temp, *tb, in, out, (uint64_t)0, (size_t)n,
                                 rocprim::plus<uint64_t>(), s);
}
hipError_t prim_rle_u64(void* temp, size_t* tb, const uint64_t* in, uint64_t* uniq, uint32_t* len,
                       uint64_t* n_runs, uint64_t n, hipStream_t s) {
  return rocprim::run_length_encode(temp, *tb, in, (unsigned)n, uniq, len, n_runs, s);
}

}  // namespace kma
