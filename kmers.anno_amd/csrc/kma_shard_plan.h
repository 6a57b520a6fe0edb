// kma_shard_plan.h — the plan of one host protein shard call (kma_abi_proteins.cpp,
// protein_shard): how its proteins are cut into pieces (one kernel each), how the packed stream
// of a streamed call is cut into copy segments and packing chunks, and where each output array
// lies in the call's output block. Integer arithmetic on the offsets only, no HIP:
// host/shard_plan_check.cpp checks it on the CPU (tests/test_shard_plan.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace kma {
namespace host {

constexpr int kMaxPieces = 16;  // host protein calls: H2D / kernel pipeline depth (events)

// Piece i is proteins [pbeg[i], pbeg[i + 1]) of the shard; a piece may be empty.
struct PiecePlan {
  int n_pieces = 1;
  uint32_t pbeg[kMaxPieces + 1] = {0};
};

// hoff: the shard's n + 1 offsets rebased to 0 (hoff[n] = nres). One piece per piece_min
// residues, at most max_pieces (and kMaxPieces); a piece starts at the first protein starting at
// or after its residue target. Equal targets, or with `ramp` and 4 pieces or more weights 1, 2,
// 4, ..., 4, 2, 1: a small first piece starts the link early and a small last piece shortens the
// tail behind the last copy ("The host call").
inline PiecePlan plan_pieces(const uint64_t* hoff, uint32_t n, uint64_t nres, uint64_t piece_min,
                             uint64_t max_pieces, bool ramp) {
  PiecePlan p;
  p.n_pieces = (int)std::max<uint64_t>(
      1, std::min<uint64_t>(std::min<uint64_t>(max_pieces, kMaxPieces), nres / piece_min));
  uint64_t wsum = 0, wcum[kMaxPieces + 1] = {0};
  for (int i = 0; i < p.n_pieces; ++i) {
    const int edge = std::min(i, p.n_pieces - 1 - i);
    wsum += !ramp || p.n_pieces < 4 ? 1u : (1u << std::min(edge, 2));
    wcum[i + 1] = wsum;
  }
  for (int i = 1; i < p.n_pieces; ++i) {
    const uint64_t target = nres * wcum[i] / wsum;
    p.pbeg[i] = (uint32_t)(std::lower_bound(hoff + p.pbeg[i - 1], hoff + n, target) - hoff);
  }
  p.pbeg[p.n_pieces] = n;
  return p;
}

// Streamed staging, in stream groups (64 residues, 40 bytes): the stream is packed in chunks of
// chunk_groups and copied in segments of at most seg_groups, the first ones smaller
// (first_seg_groups, doubling) so that the link starts early. Segments of >= 2.6 MB keep the
// copies near the one-copy rate (2 MiB copies: 42 vs 51 GB/s).
struct SegShape {
  uint64_t chunk_groups = 1u << 12, first_seg_groups = 1u << 16, seg_groups = 1u << 18;
};
struct Seg {
  uint64_t g0, g1;
  int piece;
  bool last;  // the piece's last segment: its kernel follows the copy
  uint32_t chunks;
};
struct SegPlan {
  std::vector<Seg> segs;
  std::vector<uint32_t> chunk_seg;  // chunk -> segment
  std::vector<uint64_t> chunk_g0;   // chunk -> first group
};

// Segments tile [0, n_groups) in order and never cross a piece boundary; the group holding a
// boundary goes with the earlier piece, so a piece's last segment ends at or after the group of
// its last residue. Every piece has a last segment (its kernel is launched behind it), if need
// be one without groups or chunks.
inline SegPlan plan_segments(const PiecePlan& pieces, const uint64_t* hoff, uint64_t n_groups,
                             SegShape shape = {}) {
  SegPlan p;
  uint64_t g = 0;
  for (int i = 0; i < pieces.n_pieces; ++i) {
    // (max(g, ...) never binds while offsets and pbeg do not decrease: the loop's guard only)
    const uint64_t g1 =
        i + 1 < pieces.n_pieces
            ? std::max(g, std::min(n_groups, (hoff[pieces.pbeg[i + 1]] + 63) / 64))
            : n_groups;
    do {
      const uint64_t want = std::min(
          shape.seg_groups, shape.first_seg_groups << std::min<size_t>(p.segs.size(), 2));
      const uint64_t e = std::min(g1, g + want);
      uint32_t nch = 0;
      for (uint64_t ch = g; ch < e; ch += shape.chunk_groups, ++nch) {
        p.chunk_seg.push_back((uint32_t)p.segs.size());
        p.chunk_g0.push_back(ch);
      }
      p.segs.push_back({g, e, i, e == g1, nch});
      g = e;
    } while (g < g1);
  }
  return p;
}

// The output block of a shard of n proteins (device and pinned host alike), in bytes:
// [fid i32 x n | count i32 x n | tally u32 x n_fid, if asked for | status u8 x n].
struct ShardLayout {
  uint32_t n, n_fid;
  bool tally;
  uint64_t fid_at, count_at, tally_at, status_at, out_bytes;
  ShardLayout(uint32_t n, uint32_t n_fid, bool tally)
      : n(n), n_fid(n_fid), tally(tally), fid_at(0), count_at(n * 4ull), tally_at(n * 8ull),
        status_at(n * 8ull + (tally ? n_fid * 4ull : 0)), out_bytes(status_at + n + 16) {}
};

}  // namespace host
}  // namespace kma
