// kma_hashindex.h — the hash annotator's resident prototype index (kma_hashindex.hip), shared
// with the C-ABI layer (kma_abi_ops.cpp: kma_proto_index_create, kma_hash_annotate_indexed) and
// with the host check program (host/hashindex_check.cpp), which runs a serial model of one block
// of the accumulate kernel from the pieces below under sanitizers. Not part of the public ABI
// (see include/kmeranno.h).
//
// The index of a prototype file: the sorted unique window keys of all prototypes, per key its
// postings (the prototypes whose ProteinKmers set holds it, ascending), and every prototype's
// set size. A genome protein is scored by one workgroup: its distinct keys are looked up in the
// unique keys, the postings of the matched keys are counted per prototype in an open-addressed
// LDS table (the count IS the number of shared distinct kmers), and the table is swept for the
// similarities. A protein with more distinct candidate prototypes than the table may hold (CAP)
// is scored in prototype ranges: [0, n_proto) is split at its midpoint until a range fits.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kma {

constexpr uint32_t kHashEmpty = 0xFFFFFFFFu;  // free slot of the id table; "no prototype"
constexpr uint32_t kHashBlock = 256;          // threads per genome protein; keys per chunk
// Distinct prototypes per scored range. Measured on c5's 1M prototypes against 4,000-protein
// genomes at 512 / 1024 / 2048.
constexpr uint32_t kHashCapDefault = 1024;
constexpr uint32_t kHashCapMax = 2048;
// [0, 2^32) halves to width 1 in 32 steps; a depth-first walk keeps one sibling per level.
constexpr uint32_t kHashStackDepth = 34;

// Slots of the table for a CAP: a power of two, at most half full at CAP, and with room for the
// inserts in flight when the distinct count passes CAP (each of the block's threads checks the
// count before it claims a slot, so at most kHashBlock claims follow the one that passed CAP):
// a free slot always remains and a probe ends.
__host__ __device__ inline uint32_t hash_table_slots(uint32_t cap) {
  const uint32_t need = 2u * cap > cap + 2u * kHashBlock ? 2u * cap : cap + 2u * kHashBlock;
  uint32_t t = 64;
  while (t < need) t <<= 1;
  return t;
}
__host__ __device__ inline uint32_t hash_log2(uint32_t pow2) {
  uint32_t b = 0;
  while ((1u << b) < pow2) ++b;
  return b;
}
// First slot probed for a prototype in a table of 2^bits slots (bits >= 1); the probe is linear.
__host__ __device__ inline uint32_t hash_slot(uint32_t proto, uint32_t bits) {
  return (proto * 0x9E3779B1u) >> (32u - bits);
}

// First position in the ascending postings [b, e) whose prototype is >= bound.
__host__ __device__ inline uint32_t postings_lower_bound(const uint32_t* postings, uint32_t b,
                                                         uint32_t e, uint32_t bound) {
  while (b < e) {
    const uint32_t mid = b + ((e - b) >> 1);
    if (postings[mid] < bound) b = mid + 1; else e = mid;
  }
  return b;
}

// Index i of the exclusive prefix pre[0 .. n] (pre[0] = 0, non-decreasing) with
// pre[i] <= j < pre[i + 1], for j < pre[n]: the key of flattened posting j of a chunk.
__host__ __device__ inline uint32_t prefix_owner(const uint32_t* pre, uint32_t n, uint32_t j) {
  uint32_t lo = 0, hi = n;  // pre[lo] <= j < pre[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (pre[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

// Prototype ranges [lo, hi) still to score, on storage of the caller (LDS on the device: the
// stack is block-uniform). An overflowing range is replaced by its halves, the lower on top.
struct HashRangeStack {
  uint32_t* lo;
  uint32_t* hi;
  uint32_t n;
  __host__ __device__ void init(uint32_t* lo_, uint32_t* hi_, uint32_t n_proto) {
    lo = lo_, hi = hi_, n = 1;
    lo[0] = 0, hi[0] = n_proto;
  }
  __host__ __device__ bool pop(uint32_t* l, uint32_t* h) {
    if (!n) return false;
    --n;
    *l = lo[n], *h = hi[n];
    return true;
  }
  // Only ranges wider than CAP >= 1 overflow: both halves are non-empty.
  __host__ __device__ void split(uint32_t l, uint32_t h) {
    const uint32_t mid = l + ((h - l) >> 1);
    lo[n] = mid, hi[n] = h;
    lo[n + 1] = l, hi[n + 1] = mid;
    n += 2;
  }
};

// The proposal rule over (similarity bits, prototype): a strictly greater similarity wins and,
// on equal similarity, the smaller prototype index (earlier prototypes win ties). Similarities
// are positive doubles, whose bits order as they do; kHashEmpty is "none" and loses to anything.
__host__ __device__ inline bool hash_better(uint64_t bits_a, uint32_t id_a, uint64_t bits_b,
                                            uint32_t id_b) {
  if (id_a == kHashEmpty) return false;
  if (id_b == kHashEmpty) return true;
  return bits_a > bits_b || (bits_a == bits_b && id_a < id_b);
}

// shared / (|A| + |B| - shared), the double expression of kma_hashanno.hip's sim_of.
__host__ __device__ inline double hash_similarity(uint32_t psize, uint32_t gsize, uint32_t c) {
  const double uni = (double)psize + (double)gsize - (double)c;
  return (double)c / uni;
}

struct HashIndexArgs {
  // the index
  const uint64_t* ukeys;     // n_u sorted unique keys
  const uint32_t* pstart;    // n_u + 1 posting starts
  const uint32_t* postings;  // prototypes, ascending per key
  const uint32_t* psize;     // distinct kmers per prototype
  uint64_t n_u;
  uint32_t n_proto;
  // the genome: segment-sorted window keys of its proteins
  const uint64_t* gsorted;
  const uint8_t* gfirst;     // first occurrence of a distinct key
  const uint64_t* goff;      // n_genome + 1 positions
  const uint32_t* gsize;     // distinct kmers per protein
  uint64_t n_gpos;
  uint32_t n_genome;
  uint32_t* gmatch;          // per position: its key's index in ukeys, or kHashEmpty
  // scoring
  double min_sim;
  uint32_t cap;              // distinct prototypes per range, 1 .. kHashCapMax
  uint32_t* out_count;       // per prototype (zeroed): proteins with sim >= min_sim
  int32_t* out_best;         // per protein: written by its block
  double* out_sim;
  unsigned long long* stats; // 3 (zeroed): proteins with candidates, split proteins, ranges
                             // scored (those holding a candidate)
};

// gmatch of every genome position.
hipError_t launch_index_lookup(const HashIndexArgs& a, hipStream_t s);
// One workgroup per genome protein: accumulate, score, publish.
hipError_t launch_index_score(const HashIndexArgs& a, hipStream_t s);

}  // namespace kma
