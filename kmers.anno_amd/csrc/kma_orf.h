// kma_orf.h — the projector's ORF index (kma_orf.hip) shared with the C-ABI layer (kma_abi_ops.cpp).
// Not part of the public ABI (see include/kmeranno.h, kma_orf_index_create / kma_extend_proposals).
//
// Layout. A contig of n bases has cnt = ceil(n / 3) slots per (strand, frame): slot (s, f, j)
// stands for strand position p = f + 3 j (s = 0: '+', the contig as given; s = 1: '-', its
// reverse complement) and lives at
//     2 hoff[c] + s 3 cnt + f cnt + j,        hoff[c] = sum of 3 cnt over the contigs before c,
// so every (contig, strand, frame) is one contiguous segment and walking a frame is walking a
// segment. Positions p > n - 3 (no whole codon) are slots of class "other".
//
// Both index arrays hold one word per slot: bit 31 is the scan's segment flag (meaningless after
// the build), bits 0..30 a strand position or kOrfNone:
//     stop_at[slot]   smallest in-frame stop position >= p                  (reverse min-scan)
//     start_at[slot]  smallest start position q <= p with no stop in [q, p]  (forward min-scan;
//                     a stop restarts the segment and itself yields none)
// Both are the same scan: positions grow along a segment, so "first since the last restart" is
// a minimum, and OrfScanOp is the usual segmented-scan operator with the flag in the value.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kmeranno.h"

namespace kma {

constexpr uint32_t kOrfNone = 0x7FFFFFFFu;  // no position (total bases < 2^31)
constexpr uint32_t kOrfFlag = 0x80000000u;  // the scan restarts at this slot
// Codon sets as bit masks over the 6-bit codon code b0 << 4 | b1 << 2 | b2 (A C G T = 0 1 2 3).
constexpr uint64_t kOrfStarts = 1ull << 14 | 1ull << 46 | 1ull << 62;  // ATG GTG TTG
constexpr uint64_t kOrfStops2 = 1ull << 48 | 1ull << 50;               // TAA TAG (code 4)
constexpr uint64_t kOrfStops3 = kOrfStops2 | 1ull << 56;               // + TGA (codes 1, 11)
enum : uint32_t { kOrfOther = 0, kOrfStart = 1, kOrfStop = 2 };

// A base folded to 2 bits, or 4 for anything but ACGT / acgt (never part of a start or stop).
__host__ __device__ inline uint32_t orf_fold(uint8_t b) {
  const uint32_t u = b & 0xDFu;
  return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}
__host__ __device__ inline uint32_t orf_class(uint32_t code, uint64_t stops) {
  return (stops >> code) & 1u ? kOrfStop : (kOrfStarts >> code) & 1u ? kOrfStart : kOrfOther;
}
__host__ __device__ inline uint32_t orf_frame_slots(uint32_t n) { return (n + 2u) / 3u; }

struct OrfScanOp {  // a = the earlier slots' value, b = the later one's
  __host__ __device__ uint32_t operator()(uint32_t a, uint32_t b) const {
    if (b & kOrfFlag) return b;
    const uint32_t va = a & kOrfNone, vb = b & kOrfNone;
    return (a & kOrfFlag) | (va < vb ? va : vb);
  }
};

struct OrfBuildArgs {
  const uint8_t* dna;       // contig c is dna[offsets[c] .. offsets[c + 1])
  const uint64_t* offsets;  // n_contig + 1
  const uint64_t* hoff;     // n_contig + 1: slots per strand before contig c
  uint32_t n_contig;
  uint64_t half;            // hoff[n_contig]; the arrays hold 2 half slots
  uint64_t stops;           // kOrfStops2 / kOrfStops3
  uint32_t* stop_at;        // out: the scans' operands
  uint32_t* start_at;
};

// The operands of one '+' slot t (in [0, half), counted per strand across contigs) and of the
// '-' slot computed from the same three bytes: the '-' codon at strand position n - 3 - p is the
// reverse complement of the '+' codon at p. Slots without a whole codon pair with themselves.
__host__ __device__ inline void orf_classify(const OrfBuildArgs& a, uint64_t t) {
  uint32_t lo = 0, hi = a.n_contig;  // the contig: hoff[lo] <= t < hoff[lo + 1]
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a.hoff[mid] <= t) lo = mid; else hi = mid;
  }
  const uint64_t off = a.offsets[lo];
  const uint32_t n = (uint32_t)(a.offsets[lo + 1] - off);
  const uint32_t cnt = orf_frame_slots(n);
  const uint32_t u = (uint32_t)(t - a.hoff[lo]);
  const uint32_t f = u / cnt, j = u - f * cnt, p = f + 3u * j;
  const bool whole = (uint64_t)p + 3u <= n;
  uint32_t kp = kOrfOther, km = kOrfOther, q = p;
  if (whole) {
    const uint8_t* d = a.dna + off + p;
    const uint32_t x0 = orf_fold(d[0]), x1 = orf_fold(d[1]), x2 = orf_fold(d[2]);
    if (!((x0 | x1 | x2) & 4u)) {
      kp = orf_class(x0 << 4 | x1 << 2 | x2, a.stops);
      km = orf_class((3u - x2) << 4 | (3u - x1) << 2 | (3u - x0), a.stops);
    }
    q = n - 3u - p;
  }
  const uint64_t plus = 2 * a.hoff[lo] + u;
  a.start_at[plus] = ((j == 0 || kp == kOrfStop) ? kOrfFlag : 0u) | (kp == kOrfStart ? p : kOrfNone);
  a.stop_at[plus] = (j + 1 == cnt ? kOrfFlag : 0u) | (kp == kOrfStop ? p : kOrfNone);
  const uint32_t fq = q % 3u, jq = q / 3u;
  const uint64_t minus = 2 * a.hoff[lo] + 3ull * cnt + (uint64_t)fq * cnt + jq;
  a.start_at[minus] = ((jq == 0 || km == kOrfStop) ? kOrfFlag : 0u) | (km == kOrfStart ? q : kOrfNone);
  a.stop_at[minus] = (jq + 1 == cnt ? kOrfFlag : 0u) | (km == kOrfStop ? q : kOrfNone);
}

struct OrfExtendArgs {
  const int32_t* len;       // n_contig contig lengths
  const uint64_t* hoff;
  const uint32_t* stop_at;
  const uint32_t* start_at;
  const kma_proposal* props;  // validated by the host: contig, strand, right - left + 1 >= 3
  uint64_t n;
  double min_strength;
  int64_t min_evidence;
  int32_t* left;
  int32_t* right;
  uint8_t* status;
  uint64_t* stats;          // 4 (device): made, rejected, weak, small
};

// Location.extend (restated, include/kmeranno.h) + PegProposalList.propose's filters for one
// proposal: two index loads, no walk.
__host__ __device__ inline uint32_t orf_extend(const OrfExtendArgs& a, const kma_proposal& pr,
                                               int32_t* out_left, int32_t* out_right) {
  *out_left = *out_right = 0;
  const int64_t n = a.len[pr.contig];
  const bool fwd = pr.strand == '+';
  const int64_t s = fwd ? (int64_t)pr.left - 1 : n - pr.right;
  const int64_t e = fwd ? (int64_t)pr.right - 1 : n - pr.left;
  if (s < 0 || e >= n) return KMA_ORF_REJECTED;
  const int64_t last = s + ((e - s + 1) / 3 - 1) * 3;  // the span's last whole codon
  const uint64_t cnt = orf_frame_slots((uint32_t)n);
  const uint64_t seg = 2 * a.hoff[pr.contig] + (fwd ? 0 : 3 * cnt) + (uint64_t)(s % 3) * cnt;
  const uint32_t stop = a.stop_at[seg + (uint64_t)(last / 3)] & kOrfNone;
  const uint32_t start = a.start_at[seg + (uint64_t)(s / 3)] & kOrfNone;
  if (stop == kOrfNone || start == kOrfNone) return KMA_ORF_REJECTED;
  const int64_t stop_end = (int64_t)stop + 2;
  const int64_t l = fwd ? (int64_t)start + 1 : n - stop_end;
  const int64_t r = fwd ? stop_end + 1 : n - (int64_t)start;
  *out_left = (int32_t)l;
  *out_right = (int32_t)r;
  if ((double)pr.evidence / (double)(r - l + 1) < a.min_strength) return KMA_ORF_WEAK;
  if ((int64_t)pr.evidence < a.min_evidence) return KMA_ORF_SMALL;
  return KMA_ORF_KEPT;
}

// Classify + the two scans, in place on a.stop_at / a.start_at (2 a.half words each), on
// `stream`. temp == nullptr: *temp_bytes = the scans' scratch.
hipError_t launch_orf_build(const OrfBuildArgs& a, void* temp, size_t* temp_bytes,
                            hipStream_t stream);
// One thread per proposal; a.stats zeroed before.
hipError_t launch_orf_extend(const OrfExtendArgs& a, hipStream_t stream);

}  // namespace kma
