// kma_sigmerge.h — the streamed signature build (kma_sig_builder, include/kmeranno.h): the state a
// key carries across batches, its combine rule, and the pieces of the union merge of two sorted
// runs. Shared by the kernels (kma_sigmerge.hip), the C-ABI layer (kma_abi_ops.cpp) and the host
// check program (host/sigmerge_check.cpp), which strings the pieces below into a serial model of
// the merge under sanitizers. Not part of the public ABI.
//
// State of a key. BuildKmerProcessor.java:137-223 keeps, per kmer, a RoleCounter made with the
// first role that hit it (good while every later hit names the same role), and afterwards deletes
// the kmers of every buffered protein. Across batches one bit ("good") is not enough, so a key's
// state is one of
//   role r      0 <= r < 2^24 - 1: every counted hit so far named r, no buffered protein holds it
//   kSigConflict  at least two different roles hit it (RoleCounter badCount > 0)
//   kSigBuffered  some buffered protein holds it (:196-208)
// ordered role < kSigConflict < kSigBuffered, and sig_combine(a, b) is a when a == b, the larger
// one when the larger is kSigConflict or kSigBuffered, else kSigConflict (two different roles).
//
// Why the result does not depend on the batches (proof sketch). Order the states by: every role
// below kSigConflict, kSigConflict below kSigBuffered, two different roles incomparable. That is
// a join-semilattice and sig_combine is its join (the least state above both): two equal states
// join to themselves, two different roles have kSigConflict as their least upper bound, and
// anything joined with a state above it gives that state. A join is associative, commutative and
// idempotent, so folding the states of a key's occurrences gives the same state however the
// occurrences are grouped into batches, whatever the order of the batches, and however often a
// batch is repeated. The fold over ALL occurrences of a key is kSigBuffered iff a buffered protein
// holds it, else kSigConflict iff two counted hits name different roles, else the one role named:
// that is a role exactly when the reference keeps the kmer (RoleCounter.isGood and not removed by
// the buffered pass), and then it is the role the reference prints. So the kept rows equal
// oracle_py.build_signatures on the concatenation of the batches.
//
// Union merge. The builder holds a resident run A (unique ascending keys with their states); a
// reduced batch B (the same shape) is merged into a second buffer. Position d of the merged order
// (ties A-first, so an equal pair is adjacent, A then B) belongs to the tile d / kSigTile; a tile
// finds the split (i, j), i + j = d, of its first and last position with sig_merge_split. Heads
// (the positions that produce an output row):
//   an A element at split (i, j) is always a head, and combines with B[j] iff j < nB and
//     B[j].key == A[i].key (sig_a_pairs);
//   a B element at split (i, j) is a head iff i == 0 or A[i - 1].key != B[j].key (sig_b_is_head).
// Both tests read an index the split gives, so a pair that straddles a tile boundary needs nothing
// of the neighbour tile. Keys are never 0 (0 marks a position without a window and is dropped
// when a batch is reduced).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kma {

constexpr uint32_t kSigConflict = 0xFFFFFFFEu;
constexpr uint32_t kSigBuffered = 0xFFFFFFFFu;
constexpr uint32_t kSigBlock = 256;           // threads of a merge block
constexpr uint32_t kSigPerThread = 8;         // consecutive merged positions per thread
constexpr uint32_t kSigTile = kSigBlock * kSigPerThread;  // merged positions per block

__host__ __device__ inline bool sig_is_role(uint32_t s) { return s < kSigConflict; }

__host__ __device__ inline uint32_t sig_combine(uint32_t a, uint32_t b) {
  if (a == b) return a;
  const uint32_t hi = a > b ? a : b;
  return hi >= kSigConflict ? hi : kSigConflict;
}

// The state of one (key, tag) pair of build_windows_kernel: tag = the role, or `neg` (kBuildNeg)
// for a window of a buffered protein.
__host__ __device__ inline uint32_t sig_state_of_tag(uint32_t tag, uint32_t neg) {
  return tag == neg ? kSigBuffered : tag;
}

// Merge path: how many elements of A precede position d (0 <= d <= nA + nB) of the merged order
// of the ascending runs A and B, ties A-first. The split is (i, d - i). Reads a[x] only for
// x < nA and b[y] only for y < nB.
__host__ __device__ inline uint64_t sig_merge_split(const uint64_t* a, uint64_t nA,
                                                    const uint64_t* b, uint64_t nB, uint64_t d) {
  uint64_t lo = d > nB ? d - nB : 0, hi = d < nA ? d : nA;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= b[d - 1 - mid]) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The same search 64 probes at a time (one per lane of a wave; a tile's two splits are searched
// in global memory, where a step is a round trip): probe l of the range [lo, hi) and the range
// left when the predicate `a[probe] <= b[d - 1 - probe]` holds for the first c probes (it is
// monotone: true below the split, false from it on). Ends with lo == hi == the split, in at most
// 6 steps for 2^32 keys.
__host__ __device__ inline uint64_t sig_probe(uint64_t lo, uint64_t hi, uint32_t l) {
  return lo + ((hi - lo) * l) / 64;
}
__host__ __device__ inline void sig_narrow(uint64_t* lo, uint64_t* hi, uint32_t c) {
  const uint64_t l0 = *lo, h0 = *hi;
  if (c == 0) {  // probe 0 is lo itself: the split
    *hi = l0;
    return;
  }
  *lo = sig_probe(l0, h0, c - 1) + 1;
  if (c < 64) *hi = sig_probe(l0, h0, c);
}
__host__ __device__ inline uint64_t sig_split_lo(uint64_t nB, uint64_t d) {
  return d > nB ? d - nB : 0;
}
__host__ __device__ inline uint64_t sig_split_hi(uint64_t nA, uint64_t d) {
  return d < nA ? d : nA;
}

// At split (i, j) with i < nA: whether the next merged element is A[i] (else it is B[j]).
__host__ __device__ inline bool sig_takes_a(uint64_t key_a, bool have_b, uint64_t key_b) {
  return !have_b || key_a <= key_b;
}

// The head rule (see above). b_there: j < nB; a_before: i > 0.
__host__ __device__ inline bool sig_a_pairs(uint64_t key_a, bool b_there, uint64_t key_bj) {
  return b_there && key_bj == key_a;
}
__host__ __device__ inline bool sig_b_is_head(bool a_before, uint64_t key_a_prev, uint64_t key_b) {
  return !a_before || key_a_prev != key_b;
}

// Tiles of a merge of nA + nB positions.
__host__ __device__ inline uint64_t sig_tiles(uint64_t nA, uint64_t nB, uint32_t tile) {
  return (nA + nB + tile - 1) / tile;
}

// One run: n unique ascending keys and their states.
struct SigRun {
  const uint64_t* keys;
  const uint32_t* states;
  uint64_t n;
};

// Batch reduce, after build_windows_kernel and the radix sort of the (key, tag) pairs: heads of
// the runs of equal non-zero keys (sig_heads_kernel), run ids (max-scan), every pair's tag folded
// into its run head's state, heads selected into (out_keys, out_states), *d_n_out = their number.
// head / run: n u32 each (head holds the head indices for the scan and the states after it),
// flags: n bytes. temp == nullptr: *temp_bytes = the need.
hipError_t launch_sig_reduce(const uint64_t* keys, const uint32_t* tags, uint64_t n,
                             uint8_t* flags, uint32_t* head, uint32_t* run, uint64_t* out_keys,
                             uint32_t* out_states, uint64_t* d_n_out, void* temp,
                             size_t* temp_bytes, hipStream_t stream);

// Union merge, pass 1: tile_off[t] = heads in the tiles before t, t = 0 .. n_tiles (tile_off has
// n_tiles + 1 entries; the last is the size of the union). temp == nullptr: *temp_bytes = the
// need for n_tiles tiles.
hipError_t launch_sig_merge_count(const SigRun& a, const SigRun& b, uint64_t* tile_cnt,
                                  uint64_t* tile_off, void* temp, size_t* temp_bytes,
                                  hipStream_t stream);
// Pass 2: the union's (key, state) rows at out_keys / out_states (tile_off[n_tiles] of each).
hipError_t launch_sig_merge_write(const SigRun& a, const SigRun& b, const uint64_t* tile_off,
                                  uint64_t* out_keys, uint32_t* out_states, hipStream_t stream);

// counts[0..3) += the states that are a role / kSigConflict / kSigBuffered (zeroed by the caller).
hipError_t launch_sig_counts(const uint32_t* states, uint64_t n, unsigned long long* counts,
                             hipStream_t stream);
// flags[i] = the state is a role.
hipError_t launch_sig_role_flags(const uint32_t* states, uint64_t n, uint8_t* flags,
                                 hipStream_t stream);

}  // namespace kma
