// kma_abi_sets.cpp — the operators of the C ABI (include/kmeranno.h) that rest on the
// ProteinKmers sets of a batch: distances / best match, hash-annotate (one-shot and against a
// resident prototype index) and the index itself. Two constructions carry all of them
// (kma_kmersets.hip): kmer_sets(), the segment-sorted window keys and distinct sizes of a batch,
// and key_postings(), the (key, owner) pairs of those sets sorted by key with their unique keys
// and range starts. Each entry checks its arguments on the host, enters its device, stages its
// batch in buffers of its own (kma_host.h), runs its launchers (kma_kmersets.hip,
// kma_distance.hip, kma_hashanno.hip, kma_hashindex.hip) on the null stream and copies the
// results back. kma_hash_annotate_indexed_device is the exception: its batch is on the device
// already, it stages and copies nothing, and it enqueues its two kernels (kma_hashsets.hip,
// kma_hashindex.hip) on the caller's stream.
#include <memory>

#include "kma_distance.h"
#include "kma_hashanno.h"
#include "kma_hashindex.h"
#include "kma_hashsets.h"
#include "kma_internal.h"
#include "kma_kmersets.h"
#include "kma_objects.h"

using namespace kma::host;

namespace {
// The ProteinKmers sets of a batch (device buffers in b): window keys, per-protein sort and
// distinct sizes; with owners, also the protein of every position and its first-occurrence flag.
struct KmerSets {
  uint8_t* res = nullptr;
  uint64_t* off = nullptr;
  uint64_t *keys = nullptr, *sorted = nullptr;
  uint32_t *size = nullptr, *owner = nullptr;
  uint8_t* first = nullptr;
  uint64_t total = 0;
};

int kmer_sets(DevBufs& b, const uint8_t* residues, const uint64_t* offsets, uint32_t n, int k,
              int end_exclusive, bool owners, uint32_t* d_alpha, KmerSets& ks) {
  DevBatch in;
  if (int rc = upload_batch(b, residues, offsets, n, 64, &in)) return rc;
  ks.res = in.bytes, ks.off = in.off, ks.total = in.total;
  const uint64_t nw = std::max<uint64_t>(ks.total, 1);
  KMA_HIP(b.alloc(&ks.keys, nw * 8));
  KMA_HIP(b.alloc(&ks.sorted, nw * 8));
  KMA_HIP(b.alloc(&ks.size, std::max<uint64_t>(n, 1) * 4));
  if (owners) {
    KMA_HIP(b.alloc(&ks.owner, nw * 4));
    KMA_HIP(b.alloc(&ks.first, nw));
  }
  KMA_HIP(kma::launch_window_keys(ks.res, ks.off, n, k, end_exclusive, ks.keys, d_alpha, nullptr));
  Scratch tmp;
  KMA_HIP(kma::launch_segmented_sort(nullptr, tmp.ask(), ks.keys, ks.sorted, ks.total, n, ks.off,
                                     ks.off + 1, 5 * k, nullptr));
  KMA_HIP(tmp.alloc(b));
  KMA_HIP(kma::launch_segmented_sort(tmp.p, tmp.bytes(), ks.keys, ks.sorted, ks.total, n, ks.off,
                                     ks.off + 1, 5 * k, nullptr));
  KMA_HIP(kma::launch_distinct(ks.sorted, ks.off, n, ks.size, nullptr));
  if (owners) KMA_HIP(kma::launch_owner_first(ks.sorted, ks.off, n, ks.owner, ks.first, nullptr));
  return KMA_OK;
}

// The postings of a batch's sets (device buffers in b): the (key, owner) pairs of distinct keys
// sorted by key with the stable radix sort, so that a key's owners ascend.
struct KeyPostings {
  uint64_t* ukeys = nullptr;   // unique keys, ascending
  uint32_t* ustart = nullptr;  // n_u + 1 range starts into owner
  uint32_t* owner = nullptr;   // n_pairs owners, by key
  const uint64_t* n_u = nullptr;  // device count of ukeys
  uint64_t n_pairs = 0;
};

// ks with owners; d_n: two zeroed device words ([0] pairs, [1] unique keys). The scratch is the
// caller's: a size query put into t before the call is served by the same buffer after it.
int key_postings(DevBufs& b, Scratch& t, const KmerSets& ks, int k, uint64_t* d_n,
                 KeyPostings& kp) {
  const uint64_t w = std::max<uint64_t>(ks.total, 1);
  uint64_t *pk, *skey;
  uint32_t *pp, *uidx;
  uint8_t* uhead;
  for (uint64_t** q : {&pk, &skey, &kp.ukeys}) KMA_HIP(b.alloc(q, w * 8));
  for (uint32_t** q : {&pp, &kp.owner, &uidx}) KMA_HIP(b.alloc(q, w * 4));
  KMA_HIP(b.alloc(&kp.ustart, (w + 1) * 4));
  KMA_HIP(b.alloc(&uhead, w));
  kp.n_u = d_n + 1;
  // every step once as a size query (the sort at its largest), then with the scratch
  for (int run = 0; run < 2; ++run) {
    void* p = run ? t.p : nullptr;
    auto tb = [&] { return run ? t.bytes() : t.ask(); };
    KMA_HIP(kma::prim_select_flagged_u64(p, tb(), ks.sorted, ks.first, pk, d_n, ks.total, nullptr));
    KMA_HIP(kma::prim_select_flagged_u32(p, tb(), ks.owner, ks.first, pp, d_n, ks.total, nullptr));
    if (run) KMA_HIP(hipMemcpy(&kp.n_pairs, d_n, 8, hipMemcpyDeviceToHost));
    KMA_HIP(kma::prim_sort_pairs_u64_u32(p, tb(), pk, skey, pp, kp.owner,
                                         run ? kp.n_pairs : ks.total, 5 * k, nullptr));
    if (!run) KMA_HIP(t.alloc(b));
  }
  KMA_HIP(kma::launch_run_heads(skey, kp.n_pairs, uhead, uidx, nullptr));
  KMA_HIP(kma::prim_select_flagged_u64(t.p, t.bytes(), skey, uhead, kp.ukeys, d_n + 1, kp.n_pairs,
                                       nullptr));
  KMA_HIP(kma::prim_select_flagged_u32(t.p, t.bytes(), uidx, uhead, kp.ustart, d_n + 1, kp.n_pairs,
                                       nullptr));
  KMA_HIP(kma::launch_set_end(kp.ustart, d_n + 1, kp.n_pairs, nullptr));
  return KMA_OK;
}

// One side of the hash annotator (`what` names it in the messages).
int check_side(const uint8_t* residues, const uint64_t* offsets, uint32_t n, const char* what) {
  if (n && (!residues || !offsets)) return fail(KMA_E_INVALID, "null %s", what);
  const std::string too_long = std::string("more than 2^31 ") + what + " residues";
  return check_offsets(offsets, n, what, 1ull << 31, too_long.c_str());
}

// What kma_hash_annotate and kma_hash_annotate_indexed check alike, in their order, and the
// reset of their outputs. The prototype side is checked when the call brings one (the indexed
// call's was checked when its index was built).
int begin_hash_annotate(double min_sim, const uint8_t* gres, const uint64_t* goff, uint32_t n_gp,
                        bool proto_side, const uint8_t* pres, const uint64_t* poff, uint32_t n_pt,
                        int32_t* out_best, double* out_sim, uint32_t* out_count) {
  if (!(min_sim >= 0.0 && min_sim < 1.0))
    return fail(KMA_E_INVALID, "Minimum similarity score must be between 0 and 1.");
  if ((n_gp && (!out_best || !out_sim)) || (n_pt && !out_count))
    return fail(KMA_E_INVALID, "null output");
  if (int rc = check_side(gres, goff, n_gp, "genome protein")) return rc;
  if (proto_side)
    if (int rc = check_side(pres, poff, n_pt, "prototype")) return rc;
  for (uint32_t i = 0; i < n_gp; ++i) {
    out_best[i] = -1;
    out_sim[i] = 0.0;
  }
  if (n_pt) std::memset(out_count, 0, n_pt * 4ull);
  return KMA_OK;
}
}  // namespace

extern "C" {

// ---- ProteinKmers.distance (GeneCopyProcessor.java:129-162) ------------------------------------
int kma_protein_distances(const uint8_t* residues, const uint64_t* offsets, uint32_t n_seq, int k,
                          uint32_t flags, const uint32_t* pair_a, const uint32_t* pair_b,
                          uint64_t n_pairs, int device, uint32_t* out_sim, uint32_t* out_size,
                          double* out_dist) {
  if (k < 2 || k > 12) return fail(KMA_E_INVALID, "kmer size %d outside 2..12", k);
  if (flags & ~KMA_F_END_EXCLUSIVE) return fail(KMA_E_INVALID, "bad flags");
  if (n_pairs && (!pair_a || !pair_b || !out_sim)) return fail(KMA_E_INVALID, "null argument");
  if (n_seq && (!residues || !offsets)) return fail(KMA_E_INVALID, "null argument");
  for (uint64_t i = 0; i < n_pairs; ++i)
    if (pair_a[i] >= n_seq || pair_b[i] >= n_seq)
      return fail(KMA_E_INVALID, "pair %llu indexes a protein >= %u", (unsigned long long)i,
                  n_seq);
  if (int rc = check_offsets(offsets, n_seq, "", 1ull << 31,
                             "more than 2^31 residues in one call"))
    return rc;
  if (n_seq == 0 || (n_pairs == 0 && !out_size)) return KMA_OK;
  DeviceScope ds(device);
  if (int rc = ds.entered()) return rc;
  DevBufs b;
  uint32_t *d_pa, *d_pb, *d_sim;
  const uint64_t np = std::max<uint64_t>(n_pairs, 1);
  KMA_HIP(b.alloc(&d_pa, np * 4));
  KMA_HIP(b.alloc(&d_pb, np * 4));
  KMA_HIP(b.alloc(&d_sim, np * 4));
  if (n_pairs) {
    KMA_HIP(hipMemcpy(d_pa, pair_a, n_pairs * 4, hipMemcpyHostToDevice));
    KMA_HIP(hipMemcpy(d_pb, pair_b, n_pairs * 4, hipMemcpyHostToDevice));
  }
  AlphabetFlag alpha;
  if (int rc = alpha.init(b)) return rc;
  KmerSets ks;  // (no owners: the pair kernel finds the first occurrences itself)
  if (int rc = kmer_sets(b, residues, offsets, n_seq, k, (flags & KMA_F_END_EXCLUSIVE) ? 1 : 0,
                         false, alpha.d, ks))
    return rc;
  if (n_pairs)
    KMA_HIP(kma::launch_pairs(ks.sorted, ks.off, ks.size, ks.sorted, ks.off, ks.size, d_pa, d_pb,
                              n_pairs, d_sim, nullptr));
  if (int rc = alpha.check()) return rc;
  std::vector<uint32_t> size(n_seq);
  KMA_HIP(hipMemcpy(size.data(), ks.size, n_seq * 4ull, hipMemcpyDeviceToHost));
  if (out_size) std::memcpy(out_size, size.data(), n_seq * 4ull);
  if (n_pairs) KMA_HIP(hipMemcpy(out_sim, d_sim, n_pairs * 4, hipMemcpyDeviceToHost));
  if (out_dist)
    for (uint64_t i = 0; i < n_pairs; ++i) {
      // SequenceKmers.distance restated: 1 - similarity / union, 1.0 when nothing is shared
      const uint32_t sim = out_sim[i];
      const double uni = (double)size[pair_a[i]] + (double)size[pair_b[i]] - (double)sim;
      out_dist[i] = sim > 0 ? 1.0 - (double)sim / uni : 1.0;
    }
  return KMA_OK;
}

int kma_protein_best_match(const uint8_t* residues, const uint64_t* offsets, uint32_t n_seq, int k,
                           uint32_t flags, const uint32_t* query, const uint64_t* cand_off,
                           const uint32_t* cand, uint32_t n_query, double max_dist, int device,
                           int32_t* out_best, double* out_best_dist) {
  if (n_query && (!query || !cand_off || !out_best)) return fail(KMA_E_INVALID, "null argument");
  const uint64_t n_pairs = n_query ? cand_off[n_query] - cand_off[0] : 0;
  if (n_pairs && !cand) return fail(KMA_E_INVALID, "null argument");
  for (uint32_t q = 0; q < n_query; ++q)
    if (cand_off[q + 1] < cand_off[q]) return fail(KMA_E_INVALID, "cand_off decreases at %u", q);
  std::vector<uint32_t> pa(n_pairs), pb(n_pairs), sim(n_pairs);
  std::vector<double> dist(n_pairs);
  for (uint32_t q = 0; q < n_query; ++q)
    for (uint64_t i = cand_off[q]; i < cand_off[q + 1]; ++i) {
      pa[i - cand_off[0]] = query[q];
      pb[i - cand_off[0]] = cand[i];
    }
  if (int rc = kma_protein_distances(residues, offsets, n_seq, k, flags, pa.data(), pb.data(),
                                     n_pairs, device, sim.data(), nullptr, dist.data()))
    return rc;
  // GeneCopyProcessor.java:135-146: fDist = maxDist; for each candidate in order,
  // if (f2Dist <= fDist) { fDist = f2Dist; found = f2; }
  for (uint32_t q = 0; q < n_query; ++q) {
    double best = max_dist;
    int32_t found = -1;
    for (uint64_t i = cand_off[q]; i < cand_off[q + 1]; ++i) {
      const double d = dist[i - cand_off[0]];
      if (d <= best) {
        best = d;
        found = (int32_t)cand[i];
      }
    }
    out_best[q] = found;
    if (out_best_dist) out_best_dist[q] = best;
  }
  return KMA_OK;
}

int kma_hash_annotate(const uint8_t* gres, const uint64_t* goff, uint32_t n_gp,
                      const uint8_t* pres, const uint64_t* poff, uint32_t n_pt, int k,
                      double min_sim, int device, int32_t* out_best, double* out_sim,
                      uint32_t* out_count) {
  if (k < 2 || k > 12) return fail(KMA_E_INVALID, "kmer size %d outside 2..12", k);
  if (int rc = begin_hash_annotate(min_sim, gres, goff, n_gp, true, pres, poff, n_pt, out_best,
                                   out_sim, out_count))
    return rc;
  if (n_gp == 0 || n_pt == 0) return KMA_OK;
  DeviceScope ds(device);
  if (int rc = ds.entered()) return rc;
  DevBufs b;
  AlphabetFlag alpha;
  uint64_t* d_n;  // [0] genome pairs, [1] unique keys, [2] runs
  if (int rc = alpha.init(b)) return rc;
  KMA_HIP(b.alloc(&d_n, 32));
  KMA_HIP(hipMemset(d_n, 0, 32));
  KmerSets g, p;
  if (int rc = kmer_sets(b, gres, goff, n_gp, k, 0, true, alpha.d, g)) return rc;
  if (int rc = kmer_sets(b, pres, poff, n_pt, k, 0, true, alpha.d, p)) return rc;
  if (int rc = alpha.check()) return rc;
  // genome (key, protein) pairs of distinct keys, sorted by key; unique keys and ranges
  Scratch t1;  // (also the candidate scan's, below)
  KMA_HIP(kma::prim_excl_sum_u32_u64(nullptr, t1.ask(), nullptr, nullptr,
                                     std::max<uint64_t>(p.total, 1), nullptr));
  KeyPostings gk;
  if (int rc = key_postings(b, t1, g, k, d_n, gk)) return rc;
  // candidates: one (prototype, protein) per shared distinct key
  kma::HashArgs a{};
  a.n_ppos = p.total;
  a.pfirst = p.first;
  a.psorted = p.sorted;
  a.powner = p.owner;
  a.psize = p.size;
  a.ukeys = gk.ukeys;
  a.n_u = gk.n_u;
  a.ustart = gk.ustart;
  a.gprot = gk.owner;
  a.gsize = g.size;
  a.min_sim = min_sim;
  const uint64_t pw = std::max<uint64_t>(p.total, 1);
  uint64_t* coff;
  KMA_HIP(b.alloc(&a.ccount, pw * 4));
  KMA_HIP(b.alloc(&a.cu, pw * 4));
  KMA_HIP(b.alloc(&coff, pw * 8));
  a.coff = coff;
  KMA_HIP(kma::launch_cand_count(a, nullptr));
  KMA_HIP(kma::prim_excl_sum_u32_u64(t1.p, t1.bytes(), a.ccount, coff, p.total, nullptr));
  uint64_t last_off = 0;
  uint32_t last_cnt = 0;
  if (p.total) {
    KMA_HIP(hipMemcpy(&last_off, coff + p.total - 1, 8, hipMemcpyDeviceToHost));
    KMA_HIP(hipMemcpy(&last_cnt, a.ccount + p.total - 1, 4, hipMemcpyDeviceToHost));
  }
  const uint64_t n_cand = last_off + last_cnt;
  KMA_HIP(b.alloc(&a.out_count, n_pt * 4ull));
  uint64_t* best_bits;
  uint32_t* best_proto;
  KMA_HIP(b.alloc(&best_bits, n_gp * 8ull));
  KMA_HIP(b.alloc(&best_proto, n_gp * 4ull));
  KMA_HIP(b.alloc(&a.best_bits, n_gp * 8ull));
  KMA_HIP(b.alloc(&a.best_proto, n_gp * 4ull));
  KMA_HIP(hipMemset(a.out_count, 0, n_pt * 4ull));
  for (uint64_t* q : {best_bits, a.best_bits}) KMA_HIP(hipMemset(q, 0, n_gp * 8ull));
  for (uint32_t* q : {best_proto, a.best_proto}) KMA_HIP(hipMemset(q, 0xFF, n_gp * 4ull));
  // Candidates are scored in slices of whole prototypes (file order) whose sort and run-length
  // encoding stay below 2^31 elements (the int counts of the CUB-style APIs this was first written against; rocPRIM's select and sort take size_t, its run-length encode still unsigned); a slice's best per protein
  // replaces the running best only when strictly higher, so earlier prototypes keep ties.
  // KMA_OPT_HASH_SLICE (tests) lowers the slice size.
  uint64_t slice_cap = (1ull << 31) - 1;
  if (const int64_t o = opt(KMA_OPT_HASH_SLICE); o > 0)
    slice_cap = std::min<uint64_t>(slice_cap, (uint64_t)o);
  std::vector<uint64_t> cum(n_pt + 1, 0);
  if (n_cand) {
    uint64_t* d_cum;
    KMA_HIP(b.alloc(&d_cum, (n_pt + 1) * 8ull));
    KMA_HIP(kma::launch_proto_cum(coff, a.ccount, p.off, n_pt, p.total, d_cum, nullptr));
    KMA_HIP(hipMemcpy(cum.data(), d_cum, (n_pt + 1) * 8ull, hipMemcpyDeviceToHost));
  }
  std::vector<uint32_t> cut{0};  // slice boundaries in prototypes
  for (uint32_t q = 0; q < n_pt; ++q) {
    if (cum[q + 1] - cum[q] > (1ull << 31) - 1)
      return fail(KMA_E_CAPACITY, "prototype %u has %llu candidates (limit 2^31 - 1)", q,
                  (unsigned long long)(cum[q + 1] - cum[q]));
    if (q > cut.back() && cum[q + 1] - cum[cut.back()] > slice_cap) cut.push_back(q);
  }
  cut.push_back(n_pt);
  uint64_t max_slice = 0;
  for (size_t i = 0; i + 1 < cut.size(); ++i)
    max_slice = std::max(max_slice, cum[cut[i + 1]] - cum[cut[i]]);
  if (max_slice) {
    uint64_t *cand, *csorted, *runs;
    uint32_t* run_len;
    KMA_HIP(b.alloc(&cand, max_slice * 8));
    KMA_HIP(b.alloc(&csorted, max_slice * 8));
    KMA_HIP(b.alloc(&runs, max_slice * 8));
    KMA_HIP(b.alloc(&run_len, max_slice * 4));
    int pbits = 1;
    while (pbits < 32 && (1ull << pbits) < n_pt) ++pbits;
    Scratch t2;
    KMA_HIP(kma::prim_sort_keys_u64(nullptr, t2.ask(), cand, csorted, max_slice, 32 + pbits, nullptr));
    KMA_HIP(kma::prim_rle_u64(nullptr, t2.ask(), csorted, runs, run_len, d_n + 2, max_slice, nullptr));
    KMA_HIP(t2.alloc(b));
    std::vector<uint64_t> hoff(n_pt + 1);
    KMA_HIP(hipMemcpy(hoff.data(), p.off, (n_pt + 1) * 8ull, hipMemcpyDeviceToHost));
    a.cand = cand;
    a.runs = runs;
    a.run_len = run_len;
    a.n_runs = d_n + 2;
    for (size_t i = 0; i + 1 < cut.size(); ++i) {
      const uint64_t nc = cum[cut[i + 1]] - cum[cut[i]];
      if (!nc) continue;
      a.pos_lo = hoff[cut[i]] - hoff[0];
      a.pos_hi = hoff[cut[i + 1]] - hoff[0];
      a.cand_base = cum[cut[i]];
      KMA_HIP(kma::launch_cand_emit(a, nullptr));
      KMA_HIP(kma::prim_sort_keys_u64(t2.p, t2.bytes(), cand, csorted, nc, 32 + pbits, nullptr));
      KMA_HIP(kma::prim_rle_u64(t2.p, t2.bytes(), csorted, runs, run_len, d_n + 2, nc, nullptr));
      KMA_HIP(kma::launch_score(a, nc, nullptr));
      KMA_HIP(kma::launch_choose(a, nc, nullptr));
      KMA_HIP(kma::launch_merge_best(best_bits, best_proto, a.best_bits, a.best_proto, n_gp,
                                     nullptr));
    }
  }
  std::vector<uint64_t> bits(n_gp);
  std::vector<uint32_t> proto(n_gp);
  KMA_HIP(hipMemcpy(bits.data(), best_bits, n_gp * 8ull, hipMemcpyDeviceToHost));
  KMA_HIP(hipMemcpy(proto.data(), best_proto, n_gp * 4ull, hipMemcpyDeviceToHost));
  KMA_HIP(hipMemcpy(out_count, a.out_count, n_pt * 4ull, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n_gp; ++i) {
    if (proto[i] == 0xFFFFFFFFu) continue;
    std::memcpy(&out_sim[i], &bits[i], 8);
    out_best[i] = (int32_t)proto[i];
  }
  return KMA_OK;
}

// ---- the resident prototype index (kma_hashindex.hip) ------------------------------------------
// The prototype side of kma_hash_annotate, built once: ProteinKmers sets as above, then the
// (key, prototype) pairs of distinct keys sorted by key with the stable radix sort, so that a
// key's postings ascend by prototype; unique keys and posting starts (key_postings, as the genome
// side's above).
int kma_proto_index_create(const uint8_t* pres, const uint64_t* poff, uint32_t n_pt, int k,
                           int device, kma_proto_index** out) {
  if (!out) return fail(KMA_E_INVALID, "null argument");
  *out = nullptr;
  if (k < 2 || k > 12) return fail(KMA_E_INVALID, "kmer size %d outside 2..12", k);
  if (int rc = check_side(pres, poff, n_pt, "prototype")) return rc;
  if (n_pt >= (1u << 31)) return fail(KMA_E_INVALID, "2^31 prototypes or more");
  std::unique_ptr<kma_proto_index> idx(new kma_proto_index);
  idx->device = device;
  idx->k = k;
  idx->n_proto = n_pt;
  if (n_pt == 0) return *out = idx.release(), KMA_OK;
  DeviceScope ds(device);
  if (int rc = ds.entered()) return rc;
  DevBufs b;
  AlphabetFlag alpha;
  uint64_t* d_n;  // [0] pairs, [1] unique keys
  if (int rc = alpha.init(b)) return rc;
  KMA_HIP(b.alloc(&d_n, 16));
  KMA_HIP(hipMemset(d_n, 0, 16));
  KmerSets p;
  if (int rc = kmer_sets(b, pres, poff, n_pt, k, 0, true, alpha.d, p)) return rc;
  if (int rc = alpha.check()) return rc;
  Scratch t;
  KeyPostings pk;
  if (int rc = key_postings(b, t, p, k, d_n, pk)) return rc;
  const uint64_t n_pairs = pk.n_pairs;
  uint64_t n_u = 0;
  KMA_HIP(hipMemcpy(&n_u, pk.n_u, 8, hipMemcpyDeviceToHost));
  // what stays: exact-size copies (idx frees them on any early return)
  idx->n_keys = n_u;
  idx->n_postings = n_pairs;
  KMA_HIP(hipMalloc(&idx->d_keys, std::max<uint64_t>(n_u, 1) * 8));
  KMA_HIP(hipMalloc(&idx->d_start, (n_u + 1) * 4));
  KMA_HIP(hipMalloc(&idx->d_postings, std::max<uint64_t>(n_pairs, 1) * 4));
  KMA_HIP(hipMalloc(&idx->d_psize, n_pt * 4ull));
  KMA_HIP(hipMemcpy(idx->d_keys, pk.ukeys, n_u * 8, hipMemcpyDeviceToDevice));
  KMA_HIP(hipMemcpy(idx->d_start, pk.ustart, (n_u + 1) * 4, hipMemcpyDeviceToDevice));
  KMA_HIP(hipMemcpy(idx->d_postings, pk.owner, n_pairs * 4, hipMemcpyDeviceToDevice));
  KMA_HIP(hipMemcpy(idx->d_psize, p.size, n_pt * 4ull, hipMemcpyDeviceToDevice));
  KMA_HIP(hipDeviceSynchronize());
  idx->bytes = n_u * 8 + (n_u + 1) * 4 + n_pairs * 4 + n_pt * 4ull;
  *out = idx.release();
  return KMA_OK;
}

int kma_proto_index_info(const kma_proto_index* idx, struct kma_proto_index_info* out) {
  if (!idx || !out) return fail(KMA_E_INVALID, "null argument");
  out->n_proto = idx->n_proto;
  out->k = idx->k;
  out->n_keys = idx->n_keys;
  out->n_postings = idx->n_postings;
  out->bytes = idx->bytes;
  return KMA_OK;
}

int kma_proto_index_destroy(kma_proto_index* idx) {
  delete idx;
  return KMA_OK;
}

int kma_hash_annotate_indexed(const kma_proto_index* idx, const uint8_t* gres,
                              const uint64_t* goff, uint32_t n_gp, double min_sim,
                              int32_t* out_best, double* out_sim, uint32_t* out_count,
                              uint64_t* out_stats) {
  if (!idx) return fail(KMA_E_INVALID, "null index");
  const uint32_t n_pt = idx->n_proto;
  if (int rc = begin_hash_annotate(min_sim, gres, goff, n_gp, false, nullptr, nullptr, n_pt,
                                   out_best, out_sim, out_count))
    return rc;
  if (out_stats) out_stats[0] = out_stats[1] = out_stats[2] = 0;
  if (n_gp == 0 || n_pt == 0) return KMA_OK;
  DeviceScope ds(idx->device);
  if (int rc = ds.entered()) return rc;
  DevBufs b;  // the call's scratch: nothing of the index is written
  AlphabetFlag alpha;
  if (int rc = alpha.init(b)) return rc;
  KmerSets g;
  if (int rc = kmer_sets(b, gres, goff, n_gp, idx->k, 0, true, alpha.d, g)) return rc;
  if (int rc = alpha.check()) return rc;
  kma::HashIndexArgs a{};
  a.ukeys = idx->d_keys;
  a.pstart = idx->d_start;
  a.postings = idx->d_postings;
  a.psize = idx->d_psize;
  a.n_u = idx->n_keys;
  a.n_proto = n_pt;
  a.gsorted = g.sorted;
  a.gfirst = g.first;
  a.goff = g.off;
  a.gsize = g.size;
  a.n_gpos = g.total;
  a.n_genome = n_gp;
  a.min_sim = min_sim;
  const int64_t cap = opt(KMA_OPT_HASH_CAP);
  a.cap = cap > 0 ? (uint32_t)cap : kma::kHashCapDefault;
  KMA_HIP(b.alloc(&a.gmatch, std::max<uint64_t>(g.total, 1) * 4));
  KMA_HIP(b.alloc(&a.out_count, n_pt * 4ull));
  KMA_HIP(b.alloc(&a.out_best, n_gp * 4ull));
  KMA_HIP(b.alloc(&a.out_sim, n_gp * 8ull));
  KMA_HIP(b.alloc(&a.stats, 24));
  KMA_HIP(hipMemset(a.out_count, 0, n_pt * 4ull));
  KMA_HIP(hipMemset(a.stats, 0, 24));
  KMA_HIP(kma::launch_index_lookup(a, nullptr));
  KMA_HIP(kma::launch_index_score(a, nullptr));
  KMA_HIP(hipMemcpy(out_best, a.out_best, n_gp * 4ull, hipMemcpyDeviceToHost));
  KMA_HIP(hipMemcpy(out_sim, a.out_sim, n_gp * 8ull, hipMemcpyDeviceToHost));
  KMA_HIP(hipMemcpy(out_count, a.out_count, n_pt * 4ull, hipMemcpyDeviceToHost));
  if (out_stats) KMA_HIP(hipMemcpy(out_stats, a.stats, 24, hipMemcpyDeviceToHost));
  return KMA_OK;
}

// ---- the indexed call on a device-resident batch (kma_hashsets.hip) ----------------------------
uint64_t kma_hash_scratch_bytes(uint64_t n_residues, uint32_t n_genome) {
  return kma::hash_scratch_layout(n_residues, n_genome).bytes;
}

// One chain on `stream`: hash_reset_kernel (d_count and d_stats to zero), genome_sets_kernel
// (gmatch and gsize of the batch into the scratch), index_score_kernel (unchanged: it reads gmatch over the
// proteins' segments, gsize and the offsets, and writes the outputs itself).
int kma_hash_annotate_indexed_device(const kma_proto_index* idx, const uint8_t* d_residues,
                                     const uint64_t* d_offsets, uint32_t n_gp,
                                     uint64_t n_residues, double min_sim, void* d_scratch,
                                     uint64_t scratch_bytes, int32_t* d_best, double* d_sim,
                                     uint32_t* d_count, uint64_t* d_stats, void* stream) {
  if (!idx) return fail(KMA_E_INVALID, "null index");
  if (!(min_sim >= 0.0 && min_sim < 1.0))
    return fail(KMA_E_INVALID, "Minimum similarity score must be between 0 and 1.");
  if (n_residues >= (1ull << 31))
    return fail(KMA_E_INVALID, "more than 2^31 genome protein residues");
  if (n_gp == 0) return KMA_OK;
  const uint32_t n_pt = idx->n_proto;
  if (!d_residues || !d_offsets || !d_scratch) return fail(KMA_E_INVALID, "null argument");
  if (!d_best || !d_sim || !d_stats || (n_pt && !d_count))
    return fail(KMA_E_INVALID, "null output");
  if (reinterpret_cast<uintptr_t>(d_residues) & 7u)
    return fail(KMA_E_INVALID, "d_residues is not 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_scratch) & 15u)
    return fail(KMA_E_INVALID, "d_scratch is not 16-byte aligned");
  const kma::HashScratchLayout lay = kma::hash_scratch_layout(n_residues, n_gp);
  if (scratch_bytes < lay.bytes)
    return fail(KMA_E_INVALID, "scratch of %llu bytes, %llu needed",
                (unsigned long long)scratch_bytes, (unsigned long long)lay.bytes);
  DeviceScope ds(idx->device);
  if (int rc = ds.entered()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned long long* stats = reinterpret_cast<unsigned long long*>(d_stats);
  KMA_HIP(kma::launch_hash_reset(d_count, n_pt, stats, d_best, d_sim, n_pt ? 0 : n_gp, s));
  if (n_pt == 0) return KMA_OK;
  uint8_t* scratch = static_cast<uint8_t*>(d_scratch);
  kma::GenomeSetsArgs g{};
  g.res = d_residues;
  g.off = d_offsets;
  g.n_genome = n_gp;
  g.k = idx->k;
  const int64_t w = opt(KMA_OPT_HASH_LDS_KEYS);
  g.w = w > 0 ? (uint32_t)w : kma::kSetsKeysMax;
  g.ukeys = idx->d_keys;
  g.n_u = idx->n_keys;
  g.gmatch = reinterpret_cast<uint32_t*>(scratch + lay.gmatch);
  g.gsize = reinterpret_cast<uint32_t*>(scratch + lay.gsize);
  g.runs = reinterpret_cast<uint64_t*>(scratch + lay.runs);
  g.alpha = stats + 3;
  kma::HashIndexArgs a{};
  a.ukeys = idx->d_keys;
  a.pstart = idx->d_start;
  a.postings = idx->d_postings;
  a.psize = idx->d_psize;
  a.n_u = idx->n_keys;
  a.n_proto = n_pt;
  a.goff = d_offsets;
  a.gsize = g.gsize;
  a.n_gpos = n_residues;
  a.n_genome = n_gp;
  a.gmatch = g.gmatch;
  a.min_sim = min_sim;
  const int64_t cap = opt(KMA_OPT_HASH_CAP);
  a.cap = cap > 0 ? (uint32_t)cap : kma::kHashCapDefault;
  a.out_count = d_count;
  a.out_best = d_best;
  a.out_sim = d_sim;
  a.stats = stats;
  KMA_HIP(kma::launch_genome_sets(g, s));
  KMA_HIP(kma::launch_index_score(a, s));
  return KMA_OK;
}

}  // extern "C"
