// kma_hashsets.h — the genome side of the indexed hash annotator built inside a block
// (kma_hashsets.hip: genome_sets_kernel), shared with the C-ABI layer (kma_abi_sets.cpp:
// kma_hash_annotate_indexed_device, kma_hash_scratch_bytes) and with the host check program
// (host/hashsets_check.cpp), which runs a serial model of one block from the pieces below under
// sanitizers. Not part of the public ABI (see include/kmeranno.h).
//
// One workgroup per genome protein makes what index_score_kernel (kma_hashindex.hip) reads:
// gmatch, per residue position the index of one distinct window key of the protein in the
// index's unique keys (or kHashEmpty), and gsize, the size of the protein's ProteinKmers set.
// The protein's window keys come from its ASCII residues through the code LUT, W at a time (W: a
// power of two, KMA_OPT_HASH_LDS_KEYS); a chunk is sorted in LDS by a bitonic network over the
// next power of two at or above its window count, padded with kKeySentinel. A protein of at most
// W windows is one chunk: a key that differs from its predecessor is a head (a distinct key).
// A longer protein leaves every sorted chunk as a run in the scratch's key area, and a key is a
// head iff it is the first of its value in its own run and no earlier run of the protein holds it
// (binary search): every distinct key is a head exactly once, in the first run that holds it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kma {

constexpr uint32_t kSetsBlock = 256;       // threads per genome protein
constexpr uint32_t kSetsKeysMin = 64;      // KMA_OPT_HASH_LDS_KEYS: a power of two in this range
constexpr uint32_t kSetsKeysMax = 4096;    // the LDS key array (32 KB) and the default W
constexpr uint32_t kSetsCodePad = 16;      // residue codes of a chunk: W + K - 1 <= W + this

// The 5-bit code of a residue byte: 1..26 for A-Z, 27 for '*', 0 for a byte outside the alphabet
// (the LUT of window_keys_kernel, kma_kmersets.hip).
__host__ __device__ inline uint32_t sets_code(uint32_t byte) {
  return (byte >= 'A' && byte <= 'Z') ? byte - 'A' + 1u : (byte == '*' ? 27u : 0u);
}

// The key of the window of k codes at c: 5 bits per residue, the first residue highest.
__host__ __device__ inline uint64_t sets_window_key(const uint8_t* c, int k) {
  uint64_t v = 0;
  for (int j = 0; j < k; ++j) v = (v << 5) | c[j];
  return v;
}

// Windows of a protein of len residues (i = 0 .. len - k).
__host__ __device__ inline uint64_t sets_windows(uint64_t len, int k) {
  return len >= (uint64_t)k ? len - (uint64_t)k + 1 : 0;
}

// The network's size for n keys: the next power of two at or above n (1 for n <= 1).
__host__ __device__ inline uint32_t sets_padded_size(uint32_t n) {
  uint32_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

// Compare-exchange t (t < size / 2) of the bitonic step with stride j inside merges of width m
// (m = 2, 4 .. size; j = m / 2 .. 1): the lower element, its partner (lower | j), and whether
// the pair is put in ascending order.
__host__ __device__ inline uint32_t sets_step_low(uint32_t t, uint32_t j) {
  return ((t & ~(j - 1u)) << 1) | (t & (j - 1u));
}
__host__ __device__ inline bool sets_step_ascending(uint32_t low, uint32_t m) {
  return (low & m) == 0u;
}

// Whether the ascending run [run, run + n) holds v.
__host__ __device__ inline bool sets_run_holds(const uint64_t* run, uint32_t n, uint64_t v) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (run[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo < n && run[lo] == v;
}

// The head rule: key j of the sorted chunk `cur` (n keys, none the sentinel), chunk number c of
// its protein, whose earlier chunks lie as sorted runs of w keys each at runs[0 .. c * w).
__host__ __device__ inline bool sets_is_head(const uint64_t* cur, uint32_t j, const uint64_t* runs,
                                             uint32_t c, uint32_t w) {
  const uint64_t v = cur[j];
  if (j && cur[j - 1] == v) return false;
  for (uint32_t r = 0; r < c; ++r)
    if (sets_run_holds(runs + (uint64_t)r * w, w, v)) return false;
  return true;
}

// The scratch of one call: gmatch (4 B per position), gsize (4 B per protein), the runs of long
// proteins (8 B per position), each part on a 16-byte boundary.
struct HashScratchLayout {
  uint64_t gmatch, gsize, runs, bytes;
};
__host__ __device__ inline HashScratchLayout hash_scratch_layout(uint64_t n_residues,
                                                                 uint32_t n_genome) {
  auto up16 = [](uint64_t v) { return (v + 15u) & ~15ull; };
  HashScratchLayout l;
  l.gmatch = 0;
  l.gsize = up16(4 * n_residues);
  l.runs = l.gsize + up16(4ull * n_genome);
  l.bytes = l.runs + up16(8 * n_residues) + 16;
  return l;
}

struct GenomeSetsArgs {
  const uint8_t* res;     // ASCII residues; protein g is res[off[g] .. off[g + 1])
  const uint64_t* off;    // n_genome + 1
  uint32_t n_genome;
  int k;
  uint32_t w;             // keys sorted in LDS at a time: a power of two, 64 .. kSetsKeysMax
  const uint64_t* ukeys;  // the index: n_u sorted unique keys
  uint64_t n_u;
  uint32_t* gmatch;       // per position (relative to off[0])
  uint32_t* gsize;        // per protein
  uint64_t* runs;         // per position: the sorted runs of proteins of more than w windows
  unsigned long long* alpha;  // set nonzero when a window holds a byte outside the alphabet
};

// count[0 .. n_count) and stats[0 .. 4) to zero; best / sim of n_default proteins to -1 / 0.0
// (the proposals of an index of no prototypes; 0: left to the score kernel). A kernel and not
// memset nodes: a captured 16- or 32-byte memset came back as a stale 16-byte pattern on the
// second replay of its graph.
hipError_t launch_hash_reset(uint32_t* count, uint32_t n_count, unsigned long long* stats,
                             int32_t* best, double* sim, uint32_t n_default, hipStream_t s);
// One workgroup per genome protein: gmatch of its positions and its gsize.
hipError_t launch_genome_sets(const GenomeSetsArgs& a, hipStream_t s);

}  // namespace kma
