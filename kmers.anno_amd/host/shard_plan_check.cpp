// shard_plan_check — the piece and segment planning of the host protein call
// (csrc/kma_shard_plan.h) on offsets arrays alone: every plan is checked against the invariants
// the host pipeline relies on, above all that a piece's kernel is never launched before every
// stream group holding its residues has been queued for copying. Built with AddressSanitizer and
// UBSan (make build/kma_shard_plan_check); tests/test_shard_plan.py runs it. No device, no library.
#include <cstdio>
#include <string>

#include "../csrc/kma_shard_plan.h"

using namespace kma::host;

namespace {
int g_cases = 0, g_failed = 0;
std::string g_case;
struct Failed {};

// A failed check ends its case (run() goes on with the next one, so that every failing case is
// listed); the program then exits with status 1.
#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAIL %s: %s: ", g_case.c_str(), #cond);       \
      std::printf(__VA_ARGS__);                                  \
      std::printf("\n");                                         \
      throw Failed();                                            \
    }                                                            \
  } while (0)

std::vector<uint64_t> offsets_of(const std::vector<uint64_t>& lens) {
  std::vector<uint64_t> off(lens.size() + 1, 0);
  for (size_t i = 0; i < lens.size(); ++i) off[i + 1] = off[i] + lens[i];
  return off;
}

uint64_t groups(uint64_t residues) { return (residues + 63) / 64; }

// The weights rule, written out: 1, 2, 4, 4, ..., 4, 2, 1 with `ramp` from 4 pieces on.
uint64_t weight(int i, int n_pieces, bool ramp) {
  if (!ramp || n_pieces < 4) return 1;
  const int edge = i < n_pieces - 1 - i ? i : n_pieces - 1 - i;
  return edge == 0 ? 1 : edge == 1 ? 2 : 4;
}

void check_pieces(const PiecePlan& p, const std::vector<uint64_t>& hoff, uint64_t piece_min,
                  uint64_t max_pieces, bool ramp) {
  const uint32_t n = (uint32_t)hoff.size() - 1;
  const uint64_t nres = hoff[n];
  uint64_t want = nres / piece_min;
  if (want > max_pieces) want = max_pieces;
  if (want > (uint64_t)kMaxPieces) want = kMaxPieces;
  if (want < 1) want = 1;
  CHECK((uint64_t)p.n_pieces == want, "%d pieces, formula %llu", p.n_pieces,
        (unsigned long long)want);
  CHECK(p.pbeg[0] == 0, "pbeg[0] = %u", p.pbeg[0]);
  CHECK(p.pbeg[p.n_pieces] == n, "pbeg[n_pieces] = %u, n = %u", p.pbeg[p.n_pieces], n);
  uint64_t wsum = 0, wcum = 0;
  for (int i = 0; i < p.n_pieces; ++i) wsum += weight(i, p.n_pieces, ramp);
  for (int i = 1; i <= p.n_pieces; ++i) {
    CHECK(p.pbeg[i] >= p.pbeg[i - 1], "pbeg[%d] = %u < pbeg[%d] = %u", i, p.pbeg[i], i - 1,
          p.pbeg[i - 1]);
    wcum += weight(i - 1, p.n_pieces, ramp);
    if (i == p.n_pieces) break;
    const uint64_t target = nres * wcum / wsum;
    uint32_t first = 0;  // the first protein starting at or after the target
    while (first < n && hoff[first] < target) ++first;
    CHECK(p.pbeg[i] == first, "pbeg[%d] = %u, linear scan %u (target %llu)", i, p.pbeg[i], first,
          (unsigned long long)target);
  }
}

void check_segments(const SegPlan& sp, const PiecePlan& p, const std::vector<uint64_t>& hoff,
                    SegShape shape) {
  const uint64_t n_groups = groups(hoff.back());
  const std::vector<Seg>& segs = sp.segs;
  CHECK(!segs.empty(), "no segment");
  // tiling, sizes, pieces in order, `last` on exactly the final segment of every piece
  uint64_t g = 0;
  int piece = 0;
  std::vector<uint64_t> piece_end(p.n_pieces, 0);
  for (size_t k = 0; k < segs.size(); ++k) {
    const Seg& s = segs[k];
    CHECK(s.g0 == g && s.g1 >= s.g0, "segment %zu [%llu, %llu) after group %llu", k,
          (unsigned long long)s.g0, (unsigned long long)s.g1, (unsigned long long)g);
    g = s.g1;
    const uint64_t size = s.g1 - s.g0, cap = shape.first_seg_groups << (k < 2 ? k : 2);
    CHECK(size <= shape.seg_groups && size <= cap, "segment %zu of %llu groups", k,
          (unsigned long long)size);
    CHECK(s.piece == piece, "segment %zu of piece %d, expected piece %d", k, s.piece, piece);
    const bool final_of_piece = k + 1 == segs.size() || segs[k + 1].piece != s.piece;
    CHECK(s.last == final_of_piece, "segment %zu of piece %d: last = %d", k, s.piece, (int)s.last);
    if (s.last) piece_end[piece++] = s.g1;
  }
  CHECK(g == n_groups, "segments end at group %llu of %llu", (unsigned long long)g,
        (unsigned long long)n_groups);
  CHECK(piece == p.n_pieces, "%d pieces own a last segment, of %d", piece, p.n_pieces);
  // the safety property: every group holding a residue of piece i has been queued with the
  // piece's last segment
  for (int i = 0; i < p.n_pieces; ++i)
    for (uint32_t q = p.pbeg[i]; q < p.pbeg[i + 1]; ++q)
      CHECK(groups(hoff[q + 1]) <= piece_end[i],
            "protein %u of piece %d ends in group %llu, the piece's copies at %llu", q, i,
            (unsigned long long)groups(hoff[q + 1]), (unsigned long long)piece_end[i]);
  // no segment spans two pieces: a piece ends with the group holding its boundary (or where the
  // piece before it ended), the last piece with the stream
  for (int i = 0; i < p.n_pieces; ++i) {
    uint64_t end = n_groups;
    if (i + 1 < p.n_pieces) {
      end = groups(hoff[p.pbeg[i + 1]]);
      if (end > n_groups) end = n_groups;
      if (i > 0 && end < piece_end[i - 1]) end = piece_end[i - 1];
    }
    CHECK(piece_end[i] == end, "piece %d ends at group %llu, its boundary at %llu", i,
          (unsigned long long)piece_end[i], (unsigned long long)end);
  }
  // chunks: in stream order, tiling their segment in chunk_groups steps
  CHECK(sp.chunk_seg.size() == sp.chunk_g0.size(), "chunk maps of %zu and %zu entries",
        sp.chunk_seg.size(), sp.chunk_g0.size());
  size_t ci = 0;
  for (size_t k = 0; k < segs.size(); ++k) {
    const Seg& s = segs[k];
    uint32_t nch = 0;
    for (uint64_t c0 = s.g0; c0 < s.g1; c0 += shape.chunk_groups, ++nch, ++ci)
      CHECK(ci < sp.chunk_seg.size() && sp.chunk_seg[ci] == k && sp.chunk_g0[ci] == c0,
            "chunk %zu: expected segment %zu, group %llu", ci, k, (unsigned long long)c0);
    CHECK(s.chunks == nch, "segment %zu: %u chunks, %u in the chunk map", k, s.chunks, nch);
  }
  CHECK(ci == sp.chunk_seg.size(), "%zu chunks in the map, %zu in the segments",
        sp.chunk_seg.size(), ci);
}

// What a case is named for, shown on its plans: the middle boundary (piece n_pieces / 2, whose
// target is nres / 2 with and without the ramp) and the offsets.
using Reach = bool (*)(uint64_t start, uint32_t protein, const std::vector<uint64_t>& hoff);

// One offsets array under one piece_min / max_pieces / shape, with and without the ramp (two
// cases). Returns the largest segment of the two plans, in groups.
uint64_t run(const char* name, const std::vector<uint64_t>& lens, uint64_t piece_min,
             uint64_t max_pieces, SegShape shape = {4, 16, 64}, Reach reach = nullptr) {
  const std::vector<uint64_t> hoff = offsets_of(lens);
  const uint32_t n = (uint32_t)lens.size();
  uint64_t largest = 0;
  for (int ramp = 0; ramp < 2; ++ramp) {
    g_case = std::string(name) + (ramp ? " (ramp)" : " (equal)");
    ++g_cases;
    try {
      const PiecePlan p = plan_pieces(hoff.data(), n, hoff[n], piece_min, max_pieces, ramp != 0);
      check_pieces(p, hoff, piece_min, max_pieces, ramp != 0);
      const SegPlan sp = plan_segments(p, hoff.data(), groups(hoff[n]), shape);
      check_segments(sp, p, hoff, shape);
      for (const Seg& s : sp.segs) largest = std::max(largest, s.g1 - s.g0);
      if (reach) {
        CHECK(p.n_pieces >= 4 && p.n_pieces % 2 == 0, "%d pieces", p.n_pieces);
        const uint32_t mid = p.pbeg[p.n_pieces / 2];
        CHECK(mid < n && reach(hoff[mid], mid, hoff),
              "the case misses its condition: middle boundary at protein %u, residue %llu", mid,
              (unsigned long long)hoff[mid]);
      }
    } catch (const Failed&) {
      ++g_failed;
    }
  }
  return largest;
}

std::vector<uint64_t> with(std::vector<uint64_t> lens, size_t at, uint64_t a, uint64_t b) {
  lens[at] = a;
  lens[at + 1] = b;
  return lens;
}
}  // namespace

int main() {
  const uint64_t kKi = 1024;
  const SegShape small = {4, 16, 64};
  run("one protein", {100}, kKi, 8);
  run("one long protein", {70000}, kKi, 8);
  run("less than one group", {10, 20, 5}, kKi, 8);
  run("no residues, one protein", {0}, kKi, 8);
  run("no residues, three proteins", {0, 0, 0}, kKi, 8);
  // 6400 = 100 groups exactly, and one residue more: 6 pieces (6400 / 1024)
  run("whole groups", std::vector<uint64_t>(64, 100), kKi, 8);
  run("whole groups + 1", with(std::vector<uint64_t>(64, 100), 62, 100, 101), kKi, 8);
  // 256 proteins of one group each in 4 pieces: the middle boundary (target 8192, protein 128) is
  // a group edge; then protein 128 starts one residue after it (8193); then, with two residues
  // fewer in the batch (target 8191), one residue before it (8191)
  const std::vector<uint64_t> edges(256, 64);
  run("boundaries on group edges", edges, 4000, 4, small,
      [](uint64_t start, uint32_t, const std::vector<uint64_t>&) { return start == 8192; });
  run("boundary + 1", with(edges, 127, 65, 63), 4000, 4, small,
      [](uint64_t start, uint32_t, const std::vector<uint64_t>&) { return start == 8193; });
  run("boundary - 1", with(with(edges, 127, 63, 64), 200, 63, 64), 4000, 4, small,
      [](uint64_t start, uint32_t, const std::vector<uint64_t>&) { return start == 8191; });
  {
    // empty proteins: the first three, the last three, and three (131..133) that start on the
    // middle boundary's target (8192) with the first non-empty protein behind them: the boundary
    // is the first of several equal offsets
    std::vector<uint64_t> lens(265, 64);
    for (size_t i : {0, 1, 2, 131, 132, 133, 262, 263, 264}) lens[i] = 0;
    const Reach first_of_the_empty = [](uint64_t start, uint32_t q,
                                        const std::vector<uint64_t>& hoff) {
      return start == 8192 && q == 131 && hoff[q + 1] == start && hoff[q + 3] == start;
    };
    run("empty proteins", lens, 4000, 4, small, first_of_the_empty);
    run("empty proteins, 16 pieces", lens, kKi, 16, small, first_of_the_empty);
  }
  // one giant protein across most pieces: empty pieces (zero-chunk last segments), in the middle
  // and, with the giant last, at the end of the stream
  run("giant in the middle", {50, 100000, 50, 50}, kKi, 16);
  run("giant last", {50, 50, 100000}, kKi, 16);
  run("giant first", {100000, 50, 50}, kKi, 16);
  run("giant alone on a group edge", {64 * 1000}, kKi, 16);
  // 74000 residues, 72 piece_min's: the piece limit decides (1, 3, 4 where the ramp starts, 16,
  // and more than kMaxPieces asked for)
  const std::vector<uint64_t> odd(2000, 37);
  for (uint64_t max_pieces : {1, 3, 4, 5, 16, 40}) {
    const std::string name = "limit of " + std::to_string(max_pieces) + " pieces";
    run(name.c_str(), odd, kKi, max_pieces);
  }
  run("64 KiB pieces", std::vector<uint64_t>(3000, 331), 64 * kKi, 8);
  {
    // the library's shape and piece size on ~40M residues (131072 proteins of 1..611 residues):
    // the segments grow 2^16, 2^17, 2^18 and the 2^18 cap is reached
    std::vector<uint64_t> lens(1u << 17);
    uint64_t x = 12345;
    for (uint64_t& l : lens) {
      x = x * 6364136223846793005ull + 1442695040888963407ull;
      l = 1 + (x >> 33) % 611;
    }
    const uint64_t largest = run("defaults, 40M residues", lens, 16ull << 20, 8, SegShape());
    if (largest != SegShape().seg_groups) {
      std::printf("FAIL defaults, 40M residues: largest segment %llu groups\n",
                  (unsigned long long)largest);
      ++g_failed;
    }
  }
  if (g_failed) {
    std::printf("shard_plan_check: %d of %d cases or their conditions FAILED\n", g_failed, g_cases);
    return 1;
  }
  std::printf("shard_plan_check ok: %d cases\n", g_cases);
  return 0;
}
