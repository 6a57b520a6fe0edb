// sigmerge_check.cpp — host check of the streamed signature build's union merge
// (csrc/kma_sigmerge.h: sig_combine, sig_merge_split and its 64-probe form sig_probe / sig_narrow,
// sig_takes_a, sig_a_pairs, sig_b_is_head, sig_tiles), built as host code under AddressSanitizer
// and UBSan (Makefile: build/kma_sigmerge_check; tests/test_sigmerge_host.py runs it).
//
//   kma_sigmerge_check nA nB tile seed pattern
//
// Two runs of nA and nB unique ascending keys with states drawn over two roles, kSigConflict and
// kSigBuffered. pattern: 0 disjoint, B below A; 1 disjoint, B above A; 2 interleaved; 3 the same
// keys (the shorter run is a prefix of the longer); 4 the same with one more key in front of A;
// 5 the same with one more key in front of B; 6 random keys, 30% of B's taken from A.
//
// The program runs the merge kernel's walk serially, tile by tile, on heap arrays of exactly the
// sizes a block stages (1 + na + nb + 1 keys and states): both splits of the tile by the binary
// and by the 64-probe search (they must agree), every thread's own split in the staged arrays,
// its steps with the head rule and the combine, the tile's head count; then the exclusive scan of
// the counts and the write pass at the scanned positions into arrays of exactly the union's size.
// The rows must equal a std::map fold of both runs with sig_combine, in key order. Exit 0 / 1;
// 2 on bad arguments.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../csrc/kma_sigmerge.h"

namespace {

struct Run {
  std::vector<uint64_t> keys;
  std::vector<uint32_t> states;
};

int wrong(const char* what, unsigned long long at, unsigned long long got,
          unsigned long long want) {
  std::fprintf(stderr, "sigmerge_check: %s at %llu: got %llu, expected %llu\n", what, at, got,
               want);
  return 1;
}

uint32_t draw_state(std::mt19937_64& rng) {
  switch (rng() % 4) {
    case 0: return 3;
    case 1: return 7;
    case 2: return kma::kSigConflict;
    default: return kma::kSigBuffered;
  }
}

bool make_runs(uint64_t nA, uint64_t nB, int pattern, std::mt19937_64& rng, Run* A, Run* B) {
  auto fill = [&](Run* r, std::vector<uint64_t> k) {
    std::sort(k.begin(), k.end());
    r->keys = std::move(k);
    r->states.resize(r->keys.size());
    for (auto& s : r->states) s = draw_state(rng);
  };
  std::vector<uint64_t> a, b;
  const uint64_t n = std::max(nA, nB);
  switch (pattern) {
    case 0:
      for (uint64_t i = 0; i < nB; ++i) b.push_back(1 + i);
      for (uint64_t i = 0; i < nA; ++i) a.push_back(1 + nB + i);
      break;
    case 1:
      for (uint64_t i = 0; i < nA; ++i) a.push_back(1 + i);
      for (uint64_t i = 0; i < nB; ++i) b.push_back(1 + nA + i);
      break;
    case 2:
      for (uint64_t i = 0; i < nA; ++i) a.push_back(2 + 2 * i);
      for (uint64_t i = 0; i < nB; ++i) b.push_back(3 + 2 * i);
      break;
    case 3: case 4: case 5:
      for (uint64_t i = 0; i < nA; ++i) a.push_back(10 + 3 * i);
      for (uint64_t i = 0; i < nB; ++i) b.push_back(10 + 3 * i);
      if (pattern == 4 && nA) a.back() = 5;  // (one key moved to the front: the count stays nA)
      if (pattern == 5 && nB) b.back() = 5;
      break;
    case 6: {
      std::set<uint64_t> sa, sb;
      while (sa.size() < nA) sa.insert(1 + rng() % (16 * n + 16));
      a.assign(sa.begin(), sa.end());
      while (sb.size() < nB) {
        if (nA && rng() % 10 < 3) sb.insert(a[rng() % nA]);
        else sb.insert(1 + rng() % (16 * n + 16));
      }
      b.assign(sb.begin(), sb.end());
      break;
    }
    default: return false;
  }
  fill(A, a);
  fill(B, b);
  return true;
}

// The 64-probe search of a tile's split, lane by lane.
uint64_t wave_split(const Run& A, const Run& B, uint64_t d, uint64_t* steps) {
  const uint64_t nA = A.keys.size(), nB = B.keys.size();
  uint64_t lo = kma::sig_split_lo(nB, d), hi = kma::sig_split_hi(nA, d);
  while (lo < hi) {
    uint32_t c = 0;
    bool seen_false = false;
    for (uint32_t l = 0; l < 64; ++l) {
      const uint64_t m = kma::sig_probe(lo, hi, l);
      if (m < lo || m >= hi) std::exit(wrong("probe outside its range", d, m, hi));
      const bool before = A.keys.at(m) <= B.keys.at(d - 1 - m);
      if (before && seen_false) std::exit(wrong("predicate not monotone", d, l, 0));
      seen_false = seen_false || !before;
      c += before;
    }
    kma::sig_narrow(&lo, &hi, c);
    ++*steps;
  }
  return lo;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: kma_sigmerge_check nA nB tile seed pattern\n");
    return 2;
  }
  const uint64_t nA = std::strtoull(argv[1], nullptr, 10), nB = std::strtoull(argv[2], nullptr, 10);
  const uint32_t tile = (uint32_t)std::strtoul(argv[3], nullptr, 10);
  const uint64_t seed = std::strtoull(argv[4], nullptr, 10);
  const int pattern = std::atoi(argv[5]);
  if (tile == 0 || tile > (1u << 16) || nA > (1u << 24) || nB > (1u << 24)) {
    std::fprintf(stderr, "sigmerge_check: bad sizes\n");
    return 2;
  }
  std::mt19937_64 rng(seed);
  Run A, B;
  if (!make_runs(nA, nB, pattern, rng, &A, &B)) {
    std::fprintf(stderr, "sigmerge_check: unknown pattern %d\n", pattern);
    return 2;
  }
  const uint64_t total = nA + nB, n_tiles = kma::sig_tiles(nA, nB, tile);
  // a thread's share of a tile: the kernel's 8 positions when the tile divides, else 1
  const uint32_t per = tile % kma::kSigPerThread == 0 ? kma::kSigPerThread : 1;

  struct Row {
    uint64_t key;
    uint32_t state;
  };
  std::vector<std::vector<Row>> tile_rows(n_tiles);  // a tile's packed heads, in order
  std::vector<uint64_t> tile_cnt(n_tiles + 1, 0), tile_off(n_tiles + 1, 0);
  uint64_t steps = 0;
  for (uint64_t t = 0; t < n_tiles; ++t) {
    const uint64_t d0 = t * tile, d1 = std::min<uint64_t>(d0 + tile, total);
    const uint64_t i0 = kma::sig_merge_split(A.keys.data(), nA, B.keys.data(), nB, d0);
    const uint64_t i1 = kma::sig_merge_split(A.keys.data(), nA, B.keys.data(), nB, d1);
    if (wave_split(A, B, d0, &steps) != i0) return wrong("64-probe split", d0, 0, i0);
    if (wave_split(A, B, d1, &steps) != i1) return wrong("64-probe split", d1, 0, i1);
    if (i1 < i0 || d1 - i1 < d0 - i0) return wrong("splits not ordered", t, i1, i0);
    const uint64_t j0 = d0 - i0, j1 = d1 - i1;
    const uint32_t na = (uint32_t)(i1 - i0), nb = (uint32_t)(j1 - j0), n = na + nb;
    // the staged arrays, exactly as long as the block fills them
    std::vector<uint64_t> s_key(1 + na + nb + 1);
    std::vector<uint32_t> s_st(1 + na + nb + 1);
    s_key[0] = i0 ? A.keys.at(i0 - 1) : 0;
    for (uint32_t x = 0; x < na; ++x) s_key[1 + x] = A.keys.at(i0 + x), s_st[1 + x] = A.states.at(i0 + x);
    for (uint32_t x = 0; x < nb; ++x)
      s_key[1 + na + x] = B.keys.at(j0 + x), s_st[1 + na + x] = B.states.at(j0 + x);
    s_key[1 + na + nb] = j1 < nB ? B.keys.at(j1) : 0;
    s_st[1 + na + nb] = j1 < nB ? B.states.at(j1) : 0;
    const uint64_t* a = s_key.data() + 1;
    const uint64_t* b = a + na;
    const uint32_t* sa = s_st.data() + 1;
    const uint32_t* sb = sa + na;
    for (uint32_t thread = 0; thread * per < tile; ++thread) {
      const uint32_t ld = std::min(thread * per, n);
      uint32_t ai = (uint32_t)kma::sig_merge_split(a, na, b, nb, ld), bi = ld - ai;
      for (uint32_t e = 0; e < per && ld + e < n; ++e) {
        const uint64_t ka = s_key.at(1 + ai), kb = s_key.at(1 + na + bi);
        if (ai < na && kma::sig_takes_a(ka, bi < nb, kb)) {
          const bool pair = kma::sig_a_pairs(ka, j0 + bi < nB, kb);
          tile_rows[t].push_back({ka, pair ? kma::sig_combine(sa[ai], sb[bi]) : sa[ai]});
          ++ai;
        } else {
          if (bi >= nb) return wrong("step past the tile's B", t, bi, nb);
          if (kma::sig_b_is_head(i0 + ai > 0, s_key.at(ai), kb)) tile_rows[t].push_back({kb, sb[bi]});
          ++bi;
        }
      }
    }
    tile_cnt[t] = tile_rows[t].size();
  }
  for (uint64_t t = 0; t < n_tiles; ++t) tile_off[t + 1] = tile_off[t] + tile_cnt[t];
  const uint64_t n_out = tile_off[n_tiles];
  std::vector<uint64_t> out_keys(n_out);
  std::vector<uint32_t> out_states(n_out);
  for (uint64_t t = 0; t < n_tiles; ++t)
    for (uint64_t x = 0; x < tile_cnt[t]; ++x) {
      out_keys.at(tile_off[t] + x) = tile_rows[t][x].key;
      out_states.at(tile_off[t] + x) = tile_rows[t][x].state;
    }

  // the fold
  std::map<uint64_t, uint32_t> want;
  for (const Run* r : {&A, &B})
    for (size_t i = 0; i < r->keys.size(); ++i) {
      auto it = want.find(r->keys[i]);
      if (it == want.end()) want.emplace(r->keys[i], r->states[i]);
      else it->second = kma::sig_combine(it->second, r->states[i]);
    }
  if (n_out != want.size()) return wrong("rows of the union", 0, n_out, want.size());
  uint64_t x = 0, shared = nA + nB - n_out;
  for (const auto& kv : want) {
    if (out_keys[x] != kv.first) return wrong("key", x, out_keys[x], kv.first);
    if (out_states[x] != kv.second) return wrong("state", x, out_states[x], kv.second);
    ++x;
  }
  // the combine's laws on the four states drawn, and on a third role
  const uint32_t st[] = {3, 7, 11, kma::kSigConflict, kma::kSigBuffered};
  for (uint32_t p : st)
    for (uint32_t q : st)
      for (uint32_t r : st) {
        if (kma::sig_combine(p, p) != p) return wrong("idempotence", p, 0, p);
        if (kma::sig_combine(p, q) != kma::sig_combine(q, p)) return wrong("commutativity", p, q, 0);
        if (kma::sig_combine(kma::sig_combine(p, q), r) != kma::sig_combine(p, kma::sig_combine(q, r)))
          return wrong("associativity", p, q, r);
      }
  std::printf("sigmerge_check ok: %llu + %llu keys, %llu shared, %llu tiles of %u, %llu probe steps\n",
              (unsigned long long)nA, (unsigned long long)nB, (unsigned long long)shared,
              (unsigned long long)n_tiles, tile, (unsigned long long)steps);
  return 0;
}
