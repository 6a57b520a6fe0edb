// kma_translate.h — protein translation of genome locations (kma_translate.hip) shared with the
// C-ABI layer (kma_abi_ops.cpp). Not part of the public ABI (see include/kmeranno.h,
// kma_translate_locations).
//
// Residue r of the flat output belongs to the location i with out_off[i] <= r < out_off[i + 1]
// and is its residue j = r - out_off[i]: the codon at forward bases left + 3j .. left + 3j + 2
// ('+'), or at right - 3j, right - 3j - 1, right - 3j - 2, each complemented ('-').
//
// Base classes count in the NCBI tables' T, C, A, G order (T / U = 0, C = 1, A = 2, G = 3, any
// other byte kTrOther), so a codon's table index is b0 << 4 | b1 << 2 | b2 and the complement
// of a class is class ^ 2 (T <-> A, C <-> G); kTrOther keeps its bit under the complement.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kmeranno.h"

namespace kma {

static_assert(sizeof(kma_location) == 16, "kma_location is 16 bytes in the ABI");
constexpr uint32_t kTrOther = 4;
// ATG, GTG, TTG as bits over the table index: the start set of the ORF index (kOrfStarts).
constexpr uint64_t kTrStarts = 1ull << 35 | 1ull << 51 | 1ull << 3;
constexpr uint32_t kTrPerThread = 4;                     // one aligned dword of residues
constexpr uint32_t kTrBlock = 256;
constexpr uint32_t kTrTile = kTrBlock * kTrPerThread;    // residues per block

__host__ __device__ inline uint8_t tr_base_class(uint32_t b) {
  const uint32_t u = b & 0xDFu;  // folds case; bytes >= 128 keep bit 7 and match no letter
  return (u == 'T' || u == 'U') ? 0 : u == 'C' ? 1 : u == 'A' ? 2 : u == 'G' ? 3 : kTrOther;
}

struct TranslateArgs {
  const uint8_t* dna;        // contig c is dna[offsets[c] .. offsets[c + 1])
  const uint64_t* offsets;   // n_contig + 1
  const kma_location* locs;  // validated by the host: inside their contigs, right >= left - 1
  const uint64_t* out_off;   // n_loc + 1, out_off[0] = 0, non-decreasing
  uint64_t n_loc;
  uint64_t total;            // out_off[n_loc] > 0
  const uint8_t* code;       // 64 residues in T, C, A, G order
  uint32_t peg;              // KMA_TR_PEG: residue 0 of a location is 'M' on a start codon
  uint8_t* out;              // total residues; 4-byte aligned
};

// The largest i in [lo, hi] with off[i] <= r, given off[lo] <= r: the location that holds
// residue r, since off[i + 1] > r for that i and every empty location before it has
// off[i'] = off[i' + 1] <= r.
__host__ __device__ inline uint64_t tr_find(const uint64_t* __restrict__ off, uint64_t lo,
                                            uint64_t hi, uint64_t r) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo + 1) >> 1);
    if (off[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// One location as a thread reads it: base k of residue j is dna[p0 + dir (3 j + k)] ^ flip.
struct TrSpan {
  uint64_t beg, end;  // its residues in the flat output
  int64_t p0, dir;
  uint32_t flip;
};

__host__ __device__ inline TrSpan tr_span(const TranslateArgs& a, uint64_t i) {
  const kma_location loc = a.locs[i];
  const int64_t coff = (int64_t)a.offsets[loc.contig];
  const bool fwd = loc.strand == '+';
  TrSpan s;
  s.beg = a.out_off[i];
  s.end = a.out_off[i + 1];
  s.p0 = coff + (fwd ? loc.left : loc.right) - 1;
  s.dir = fwd ? 1 : -1;
  s.flip = fwd ? 0u : 2u;
  return s;
}

// One thread's residues r .. min(r + kTrPerThread, r_end) of a block whose residues lie in the
// locations lo .. hi; lut = tr_base_class of every byte, code = the 64 residues (LDS in the kernel).
__host__ __device__ inline void tr_thread(const TranslateArgs& a, const uint8_t* lut,
                                          const uint8_t* code, uint64_t lo, uint64_t hi,
                                          uint64_t r, uint64_t r_end) {
  if (r >= r_end) return;
  uint64_t i = tr_find(a.out_off, lo, hi, r);
  TrSpan s = tr_span(a, i);
  const uint32_t n = r_end - r < kTrPerThread ? (uint32_t)(r_end - r) : kTrPerThread;
  uint32_t word = 0;
#pragma unroll
  for (uint32_t q = 0; q < kTrPerThread; ++q) {
    if (q < n) {
      const uint64_t rq = r + q;
      if (rq >= s.end) {  // crossed into another location (and over any empty ones between)
        i = tr_find(a.out_off, i + 1, hi, rq);
        s = tr_span(a, i);
      }
      const uint64_t j = rq - s.beg;
      const uint8_t* d = a.dna + (s.p0 + s.dir * (int64_t)(3 * j));
      const uint32_t b0 = lut[d[0]] ^ s.flip;
      const uint32_t b1 = lut[d[s.dir]] ^ s.flip;
      const uint32_t b2 = lut[d[2 * s.dir]] ^ s.flip;
      uint32_t aa = 'X';
      if (!((b0 | b1 | b2) & kTrOther)) {
        const uint32_t c = b0 << 4 | b1 << 2 | b2;
        aa = (a.peg && j == 0 && ((kTrStarts >> c) & 1u)) ? (uint32_t)'M' : code[c];
      }
      word |= aa << (8 * q);
    }
  }
  if (n == kTrPerThread) {
    *reinterpret_cast<uint32_t*>(a.out + r) = word;  // r is a multiple of 4, a.out 4-byte aligned
  } else {
    for (uint32_t q = 0; q < n; ++q) a.out[r + q] = (uint8_t)(word >> (8 * q));
  }
}

// ceil(total / kTrTile) blocks on `stream`; a.total > 0.
hipError_t launch_translate(const TranslateArgs& a, hipStream_t stream);

}  // namespace kma
