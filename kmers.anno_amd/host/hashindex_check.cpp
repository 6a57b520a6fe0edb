// hashindex_check.cpp — host check of the block body of the resident prototype index's score
// kernel (csrc/kma_hashindex.h: hash_table_slots / hash_slot, postings_lower_bound,
// prefix_owner, HashRangeStack, hash_better, hash_similarity), built as host code under
// AddressSanitizer and UBSan (Makefile: build/kma_hashindex_check; tests/test_hashindex_host.py
// writes the case files and runs it).
//
//   kma_hashindex_check CASE
//   kma_hashindex_check --hash CAP [ID ...]
//
// --hash prints "slots T bits B" of hash_table_slots(CAP) and then one line "ID SLOT" of
// hash_slot(ID, B) per prototype id: tests/test_hashindex_workload.py holds its Python mirror of
// the two functions to these.
//
// CASE: u32 n_proto, u32 n_genome, u32 cap, u32 0, f64 min_sim; then per prototype and then per
// genome protein a u32 count and that many u64 window keys (any order, repeats allowed: the
// ProteinKmers set is their distinct values); then per genome protein what the writer expects:
// i32 best prototype (-1: none), u32 kmers shared with it, u32 distinct candidate prototypes.
//
// The program builds the index as kma_proto_index_create leaves it (sorted unique keys, posting
// starts, postings ascending per key, set sizes) in heap arrays of exactly those sizes, and runs
// one block's walk per genome protein serially: chunks of kHashBlock positions, the prefix of
// the posting lengths, the flattened postings into the open-addressed table, the overflow split
// on the range stack, the sweep with the running best. Every protein's best, similarity bits,
// shared count, candidate count and split flag, and every prototype's match count, must equal a
// brute-force count over all pairs, and the file's expectations. The "ok" line ends with the
// longest probe of any insert (slots looked at) and whether a probe passed from the table's last
// slot to slot 0.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/kma_hashindex.h"

namespace {

using kma::kHashBlock;
using kma::kHashEmpty;

struct Case {
  uint32_t n_proto = 0, n_genome = 0, cap = 0;
  double min_sim = 0;
  std::vector<std::vector<uint64_t>> proto, genome;  // sorted window keys, repeats kept
  std::vector<int32_t> want_best;
  std::vector<uint32_t> want_shared, want_cand;
};

bool read_keys(FILE* f, uint32_t n, std::vector<std::vector<uint64_t>>* out) {
  out->resize(n);
  for (auto& v : *out) {
    uint32_t c;
    if (std::fread(&c, 4, 1, f) != 1) return false;
    v.resize(c);
    if (c && std::fread(v.data(), 8, c, f) != c) return false;
    std::sort(v.begin(), v.end());
  }
  return true;
}

bool read_case(const char* path, Case* c) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  uint32_t head[4];
  bool ok = std::fread(head, 4, 4, f) == 4 && std::fread(&c->min_sim, 8, 1, f) == 1;
  if (ok) {
    c->n_proto = head[0], c->n_genome = head[1], c->cap = head[2];
    ok = read_keys(f, c->n_proto, &c->proto) && read_keys(f, c->n_genome, &c->genome);
  }
  c->want_best.resize(c->n_genome);
  c->want_shared.resize(c->n_genome);
  c->want_cand.resize(c->n_genome);
  for (uint32_t g = 0; ok && g < c->n_genome; ++g)
    ok = std::fread(&c->want_best[g], 4, 1, f) == 1 && std::fread(&c->want_shared[g], 4, 1, f) == 1 &&
         std::fread(&c->want_cand[g], 4, 1, f) == 1;
  std::fclose(f);
  return ok;
}

uint32_t distinct_size(const std::vector<uint64_t>& sorted) {
  uint32_t n = 0;
  for (size_t i = 0; i < sorted.size(); ++i) n += i == 0 || sorted[i] != sorted[i - 1];
  return n;
}

// Heap arrays of exactly the index's sizes: a read past one is a sanitizer error.
struct Index {
  uint64_t n_u = 0, n_post = 0;
  uint64_t* ukeys = nullptr;
  uint32_t *pstart = nullptr, *postings = nullptr, *psize = nullptr;
  ~Index() {
    std::free(ukeys), std::free(pstart), std::free(postings), std::free(psize);
  }
};

void build_index(const Case& c, Index* ix) {
  std::vector<std::pair<uint64_t, uint32_t>> pairs;  // (key, prototype) of distinct keys
  ix->psize = static_cast<uint32_t*>(std::malloc(std::max<size_t>(c.n_proto, 1) * 4));
  for (uint32_t p = 0; p < c.n_proto; ++p) {
    const auto& v = c.proto[p];
    ix->psize[p] = distinct_size(v);
    for (size_t i = 0; i < v.size(); ++i)
      if (i == 0 || v[i] != v[i - 1]) pairs.emplace_back(v[i], p);
  }
  std::stable_sort(pairs.begin(), pairs.end(),
                   [](const auto& a, const auto& b) { return a.first < b.first; });
  ix->n_post = pairs.size();
  for (size_t i = 0; i < pairs.size(); ++i) ix->n_u += i == 0 || pairs[i].first != pairs[i - 1].first;
  ix->ukeys = static_cast<uint64_t*>(std::malloc(std::max<uint64_t>(ix->n_u, 1) * 8));
  ix->pstart = static_cast<uint32_t*>(std::malloc((ix->n_u + 1) * 4));
  ix->postings = static_cast<uint32_t*>(std::malloc(std::max<uint64_t>(ix->n_post, 1) * 4));
  uint64_t u = 0;
  for (size_t i = 0; i < pairs.size(); ++i) {
    if (i == 0 || pairs[i].first != pairs[i - 1].first) {
      ix->ukeys[u] = pairs[i].first;
      ix->pstart[u++] = (uint32_t)i;
    }
    ix->postings[i] = pairs[i].second;
  }
  ix->pstart[ix->n_u] = (uint32_t)pairs.size();
}

struct Probes {
  uint32_t longest = 0;  // slots looked at by one table_add
  bool wrapped = false;  // a probe went on from slot T - 1 to slot 0
};

struct Result {
  uint32_t best = kHashEmpty, shared = 0, cand = 0, ranges = 0;
  uint64_t bits = 0;
  bool split = false;
};

// table_add of kma_hashindex.hip without its atomics.
void table_add(uint32_t* ids, uint32_t* cnt, uint32_t* distinct, uint32_t proto, uint32_t bits,
               uint32_t cap, Probes* pr) {
  const uint32_t mask = (1u << bits) - 1u;
  uint32_t h = kma::hash_slot(proto, bits);
  for (uint32_t probe = 0; probe <= mask; ++probe, h = (h + 1) & mask) {
    pr->longest = std::max(pr->longest, probe + 1);
    if (probe && h == 0) pr->wrapped = true;
    if (ids[h] == kHashEmpty) {
      if (*distinct > cap) return;
      ids[h] = proto;
      ++*distinct;
    }
    if (ids[h] == proto) {
      ++cnt[h];
      return;
    }
  }
  std::fprintf(stderr, "hashindex_check: the table filled up\n");
  std::exit(1);
}

// One block: genome protein `keys` (sorted, repeats kept) against the index.
Result run_block(const Case& c, const Index& ix, const std::vector<uint64_t>& keys,
                 std::vector<uint32_t>* out_count, Probes* pr) {
  Result r;
  const uint32_t gsize = distinct_size(keys);
  std::vector<uint32_t> gmatch(keys.size(), kHashEmpty);  // index_lookup_kernel
  for (size_t i = 0; i < keys.size(); ++i) {
    if (i && keys[i] == keys[i - 1]) continue;
    const uint64_t* at = std::lower_bound(ix.ukeys, ix.ukeys + ix.n_u, keys[i]);
    if (at != ix.ukeys + ix.n_u && *at == keys[i]) gmatch[i] = (uint32_t)(at - ix.ukeys);
  }
  const uint32_t slots = kma::hash_table_slots(c.cap), bits = kma::hash_log2(slots);
  uint32_t* ids = static_cast<uint32_t*>(std::malloc(slots * 4));
  uint32_t* cnt = static_cast<uint32_t*>(std::malloc(slots * 4));
  uint32_t* pre = static_cast<uint32_t*>(std::malloc((kHashBlock + 1) * 4));
  uint32_t* start = static_cast<uint32_t*>(std::malloc(kHashBlock * 4));
  uint32_t* s_lo = static_cast<uint32_t*>(std::malloc(kma::kHashStackDepth * 4));
  uint32_t* s_hi = static_cast<uint32_t*>(std::malloc(kma::kHashStackDepth * 4));
  kma::HashRangeStack st;
  st.init(s_lo, s_hi, c.n_proto);
  bool first = true;
  uint32_t lo, hi;
  while (st.pop(&lo, &hi)) {
    uint32_t distinct = 0;
    std::fill(ids, ids + slots, kHashEmpty);
    std::fill(cnt, cnt + slots, 0u);
    for (size_t base = 0; base < keys.size() && distinct <= c.cap; base += kHashBlock) {
      uint32_t total = 0;
      for (uint32_t t = 0; t < kHashBlock; ++t) {
        uint32_t b = 0, len = 0;
        if (base + t < keys.size() && gmatch[base + t] != kHashEmpty) {
          const uint32_t u = gmatch[base + t];
          uint32_t e = ix.pstart[u + 1];
          b = ix.pstart[u];
          if (lo) b = kma::postings_lower_bound(ix.postings, b, e, lo);
          if (hi < c.n_proto) e = kma::postings_lower_bound(ix.postings, b, e, hi);
          len = e - b;
        }
        pre[t] = total;
        start[t] = b;
        total += len;
      }
      pre[kHashBlock] = total;
      for (uint32_t j = 0; j < total; ++j) {
        const uint32_t key = kma::prefix_owner(pre, kHashBlock, j);
        table_add(ids, cnt, &distinct, ix.postings[start[key] + (j - pre[key])], bits, c.cap,
                  pr);
      }
    }
    if (first) r.cand = distinct;  // (of [0, n_proto): exact only when it did not overflow)
    first = false;
    if (distinct > c.cap) {
      r.split = true;
      st.split(lo, hi);
      if (st.n > kma::kHashStackDepth) std::fprintf(stderr, "hashindex_check: stack\n"), std::exit(1);
      continue;
    }
    if (distinct == 0) continue;
    ++r.ranges;
    for (uint32_t s = 0; s < slots; ++s) {
      if (ids[s] == kHashEmpty) continue;
      if (ids[s] < lo || ids[s] >= hi) std::fprintf(stderr, "hashindex_check: range\n"), std::exit(1);
      const double sim = kma::hash_similarity(ix.psize[ids[s]], gsize, cnt[s]);
      if (!(sim >= c.min_sim)) continue;
      ++(*out_count)[ids[s]];
      uint64_t sb;
      std::memcpy(&sb, &sim, 8);
      if (kma::hash_better(sb, ids[s], r.bits, r.best)) r.bits = sb, r.best = ids[s], r.shared = cnt[s];
    }
  }
  std::free(ids), std::free(cnt), std::free(pre), std::free(start), std::free(s_lo), std::free(s_hi);
  return r;
}

uint32_t shared_of(const std::vector<uint64_t>& a, const std::vector<uint64_t>& b) {
  uint32_t n = 0;
  size_t i = 0, j = 0;
  while (i < a.size() && j < b.size()) {
    if (a[i] < b[j]) ++i;
    else if (b[j] < a[i]) ++j;
    else {
      const uint64_t v = a[i];
      ++n;
      while (i < a.size() && a[i] == v) ++i;
      while (j < b.size() && b[j] == v) ++j;
    }
  }
  return n;
}

int wrong(uint32_t g, const char* what, long long got, long long want) {
  std::fprintf(stderr, "hashindex_check: protein %u: wrong %s: %lld, expected %lld\n", g, what, got,
               want);
  return 1;
}

// --hash CAP [ID ...]: the table of a CAP and the first slots of prototype ids in it.
int print_hash(int argc, char** argv) {
  const unsigned long cap = std::strtoul(argv[2], nullptr, 10);
  if (cap < 1 || cap > kma::kHashCapMax)
    return std::fprintf(stderr, "hashindex_check: CAP is 1..%u\n", kma::kHashCapMax), 2;
  const uint32_t slots = kma::hash_table_slots((uint32_t)cap), bits = kma::hash_log2(slots);
  std::printf("slots %u bits %u\n", slots, bits);
  for (int i = 3; i < argc; ++i) {
    const uint32_t id = (uint32_t)std::strtoul(argv[i], nullptr, 10);
    std::printf("%u %u\n", id, kma::hash_slot(id, bits));
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 3 && !std::strcmp(argv[1], "--hash")) return print_hash(argc, argv);
  if (argc != 2)
    return std::fprintf(stderr, "usage: kma_hashindex_check CASE | --hash CAP [ID ...]\n"), 2;
  Case c;
  if (!read_case(argv[1], &c) || c.cap < 1 || c.cap > kma::kHashCapMax)
    return std::fprintf(stderr, "hashindex_check: cannot read %s\n", argv[1]), 2;
  Index ix;
  build_index(c, &ix);
  std::vector<uint32_t> count(c.n_proto, 0), brute_count(c.n_proto, 0);
  uint32_t n_split = 0, n_ranges = 0;
  Probes probes;
  for (uint32_t g = 0; g < c.n_genome; ++g) {
    const Result r = run_block(c, ix, c.genome[g], &count, &probes);
    // all pairs, in file order: a proposal needs sim >= min_sim and above the current one
    const uint32_t gsize = distinct_size(c.genome[g]);
    int32_t best = -1;
    double best_sim = 0.0;
    uint32_t best_shared = 0, cand = 0;
    for (uint32_t p = 0; p < c.n_proto; ++p) {
      const uint32_t sh = shared_of(c.genome[g], c.proto[p]);
      if (!sh) continue;
      ++cand;
      const double sim = kma::hash_similarity(distinct_size(c.proto[p]), gsize, sh);
      if (!(sim >= c.min_sim)) continue;
      ++brute_count[p];
      if (best < 0 || sim > best_sim) best = (int32_t)p, best_sim = sim, best_shared = sh;
    }
    uint64_t want_bits = 0;
    if (best >= 0) std::memcpy(&want_bits, &best_sim, 8);
    const int32_t got_best = r.best == kHashEmpty ? -1 : (int32_t)r.best;
    if (got_best != best) return wrong(g, "best", got_best, best);
    if (r.bits != want_bits) return wrong(g, "similarity bits", (long long)r.bits, (long long)want_bits);
    if (r.shared != best_shared) return wrong(g, "count", r.shared, best_shared);
    if (r.split != (cand > c.cap)) return wrong(g, "split", r.split, cand > c.cap);
    if (!r.split && r.cand != cand) return wrong(g, "candidate count", r.cand, cand);
    if (got_best != c.want_best[g]) return wrong(g, "best", got_best, c.want_best[g]);
    if (r.shared != c.want_shared[g]) return wrong(g, "count", r.shared, c.want_shared[g]);
    if (cand != c.want_cand[g]) return wrong(g, "candidate count", cand, c.want_cand[g]);
    n_split += r.split;
    n_ranges += r.ranges;
  }
  for (uint32_t p = 0; p < c.n_proto; ++p)
    if (count[p] != brute_count[p]) return wrong(p, "prototype match count", count[p], brute_count[p]);
  std::printf("hashindex_check ok: %u prototypes, %u proteins, %u split, %u ranges, "
              "longest probe %u, wrapped %u\n",
              c.n_proto, c.n_genome, n_split, n_ranges, probes.longest, probes.wrapped ? 1u : 0u);
  return 0;
}
