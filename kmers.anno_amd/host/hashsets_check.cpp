// hashsets_check.cpp — host check of the block body of genome_sets_kernel (csrc/kma_hashsets.h:
// sets_code / sets_window_key, sets_windows, sets_padded_size, sets_step_low /
// sets_step_ascending, sets_run_holds / sets_is_head), built as host code under AddressSanitizer
// and UBSan (Makefile: build/kma_hashsets_check; tests/test_hashsets_host.py writes the case
// files and runs it).
//
//   kma_hashsets_check CASE
//
// CASE: u32 n_cases; then per case u32 W (keys per chunk), u32 K, u32 length, u32 the size of the
// protein's ProteinKmers set as the writer expects it, u32 whether the writer expects the
// alphabet flag, and `length` residue bytes.
//
// Per case the program runs one block's walk serially, on heap arrays of exactly the sizes the
// kernel touches: the chunk's codes (its windows' bytes only), the keys padded with the sentinel
// to sets_padded_size, every compare-exchange of the bitonic network in step order, the chunk
// left as a run when the protein has more than W windows, and the head rule for every key. The
// sorted chunk must equal std::sort's, the heads must be exactly the distinct windows of a
// brute-force set of substrings (each once), their number the file's, and the alphabet flag the
// brute-force one.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "../csrc/kma_hashsets.h"
#include "../csrc/kma_kmersets.h"

namespace {

struct Case {
  uint32_t w = 0, k = 0, want_size = 0, want_bad = 0;
  std::vector<uint8_t> res;
};

bool read_cases(const char* path, std::vector<Case>* out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  uint32_t n = 0;
  bool ok = std::fread(&n, 4, 1, f) == 1;
  for (uint32_t i = 0; ok && i < n; ++i) {
    uint32_t h[5];
    ok = std::fread(h, 4, 5, f) == 5;
    if (!ok) break;
    Case c;
    c.w = h[0], c.k = h[1], c.want_size = h[3], c.want_bad = h[4];
    c.res.resize(h[2]);
    ok = !h[2] || std::fread(c.res.data(), 1, h[2], f) == h[2];
    out->push_back(std::move(c));
  }
  std::fclose(f);
  return ok;
}

int wrong(size_t i, const char* what, unsigned long long got, unsigned long long want) {
  std::fprintf(stderr, "hashsets_check: case %zu: %s: got %llu, expected %llu\n", i, what, got,
               want);
  return 1;
}

// One block's walk over one protein. heads: the keys the block counts, in the order found.
int run_case(size_t ci, const Case& c, uint64_t* n_steps) {
  const uint32_t W = c.w;
  const int k = (int)c.k;
  const uint64_t len = c.res.size(), n_win = kma::sets_windows(len, k);
  if (W < kma::kSetsKeysMin || W > kma::kSetsKeysMax || (W & (W - 1)) || k < 2 || k > 12 ||
      c.k - 1 > kma::kSetsCodePad)
    return wrong(ci, "bad W or K", W, c.k);
  std::vector<uint64_t> runs(n_win > W ? n_win : 0);  // the scratch's key area of this protein
  std::vector<uint64_t> heads;
  bool bad = false;
  uint32_t chunk = 0;
  for (uint64_t c0 = 0; c0 < n_win; c0 += W, ++chunk) {
    const uint32_t nw = (uint32_t)std::min<uint64_t>(W, n_win - c0);
    const uint32_t n2 = kma::sets_padded_size(nw);
    if (n2 < nw || n2 > W || (n2 & (n2 - 1)) || (n2 > 1 && n2 / 2 >= nw))
      return wrong(ci, "padded size", n2, nw);
    std::vector<uint8_t> code(nw + k - 1);
    for (uint32_t i = 0; i < nw + k - 1; ++i) {
      code[i] = (uint8_t)kma::sets_code(c.res[c0 + i]);
      bad = bad || code[i] == 0;
    }
    std::vector<uint64_t> key(n2);
    for (uint32_t i = 0; i < n2; ++i)
      key[i] = i < nw ? kma::sets_window_key(code.data() + i, k) : kma::kKeySentinel;
    std::vector<uint64_t> sorted(key);
    std::sort(sorted.begin(), sorted.end());
    for (uint32_t m = 2; m <= n2; m <<= 1)
      for (uint32_t j = m >> 1; j; j >>= 1, ++*n_steps)
        for (uint32_t t = 0; t < n2 / 2; ++t) {
          const uint32_t lo = kma::sets_step_low(t, j), hi = lo | j;
          if (hi == lo || hi >= n2) return wrong(ci, "partner", hi, n2);
          const uint64_t x = key.at(lo), y = key.at(hi);
          if ((x > y) == kma::sets_step_ascending(lo, m)) key[lo] = y, key[hi] = x;
        }
    if (key != sorted) return wrong(ci, "the network does not sort chunk", chunk, 0);
    for (uint32_t j = 0; j < nw; ++j)
      if (kma::sets_is_head(key.data(), j, runs.data(), chunk, W)) heads.push_back(key[j]);
    if (!runs.empty()) std::copy(key.begin(), key.begin() + nw, runs.begin() + c0);
  }
  // brute force: the distinct substrings, and their keys by the plain rule
  std::set<std::string> subs;
  std::set<uint64_t> want_keys;
  bool want_bad = false;
  for (uint64_t i = 0; i < n_win; ++i) {
    subs.insert(std::string(c.res.begin() + i, c.res.begin() + i + k));
    uint64_t v = 0;
    for (int j = 0; j < k; ++j) {
      const uint8_t b = c.res[i + j];
      const uint32_t cd = (b >= 'A' && b <= 'Z') ? b - 'A' + 1u : (b == '*' ? 27u : 0u);
      want_bad = want_bad || cd == 0;
      v = v * 32 + cd;
    }
    want_keys.insert(v);
  }
  if (bad != want_bad || (uint32_t)bad != c.want_bad) return wrong(ci, "alphabet flag", bad, c.want_bad);
  if (bad) return 0;  // (keys of bytes without a code are not distinct per substring)
  if (heads.size() != subs.size()) return wrong(ci, "wrong size", heads.size(), subs.size());
  if (heads.size() != c.want_size) return wrong(ci, "wrong size", heads.size(), c.want_size);
  std::sort(heads.begin(), heads.end());
  if (!std::equal(heads.begin(), heads.end(), want_keys.begin(), want_keys.end()))
    return wrong(ci, "the heads are not the distinct keys", heads.size(), want_keys.size());
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: kma_hashsets_check CASE\n");
    return 2;
  }
  std::vector<Case> cases;
  if (!read_cases(argv[1], &cases)) {
    std::fprintf(stderr, "hashsets_check: cannot read %s\n", argv[1]);
    return 2;
  }
  uint64_t n_steps = 0;
  for (size_t i = 0; i < cases.size(); ++i)
    if (run_case(i, cases[i], &n_steps)) return 1;
  std::printf("hashsets_check ok: %zu cases, %llu network steps\n", cases.size(),
              (unsigned long long)n_steps);
  return 0;
}
