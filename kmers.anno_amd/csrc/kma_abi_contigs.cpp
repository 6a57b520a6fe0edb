// kma_abi_contigs.cpp — the 6-frame (contig) path of the C ABI (include/kmeranno.h): the
// workspace's contig scratch, the device entry point, and the host pipeline of
// kma_annotate_contigs / kma_connect_pegs (two passes per replica shard: count, then emit).
#include "kma_internal.h"
#include "kma_objects.h"

using namespace kma::host;

const char* const kma::host::kContigPhases[2] = {"contigs_probe_kernel", "scan_emit"};

void kma::host::free_contig_scratch(kma_workspace* ws) {
  for (void* p : {(void*)ws->d_cstage, (void*)ws->d_ccounts, (void*)ws->d_cprefix})
    if (p) (void)hipFree(p);
  ws->d_cstage = nullptr;
  ws->d_ccounts = nullptr;
  ws->d_cprefix = nullptr;
  ws->contig_cap = 0;
}

namespace {
uint64_t contig_blocks(uint64_t n_bases) {
  return std::max<uint64_t>(1, (n_bases + kma::kContigTile - 1) / kma::kContigTile);
}

// Codon table of an NCBI code as 5-bit amino-acid codes (0 = stop or ambiguous).
void codon_codes(const char* code, uint8_t out[64]) {
  for (int i = 0; i < 64; ++i)
    out[i] = (code[i] == '*' || code[i] == 'X') ? 0 : (uint8_t)(code[i] - 'A' + 1);
}

int contig_args(const kma_table* t, const Replica& r, kma_workspace* ws, const uint8_t* d_dna,
                const uint64_t* d_offsets, uint32_t n_contig, uint64_t n_bases, const char* code,
                uint32_t* d_tally, uint32_t n_fid, hipStream_t s, kma::ContigArgs* out) {
  kma::ContigArgs a{};
  a.slots = r.d_slots;
  a.n_buckets = (uint32_t)t->n_buckets;
  a.dna = d_dna;
  a.offsets = d_offsets;
  a.n_contig = n_contig;
  a.total_bases = n_bases;
  a.k = t->k;
  a.mlen = t->mlen;
  a.two_choice = t->two_choice ? 1u : 0u;
  a.staging = ws->d_cstage;
  a.block_counts = ws->d_ccounts;
  // An earlier call failed between its probe and its emit: start clean, ordered on this
  // call's stream (calls on one workspace are ordered on one stream, kmeranno.h).
  if (ws->cpending) KMA_HIP(hipMemsetAsync(ws->d_cprefix, 0, (ws->cgroups + 1) * 8, s));
  ws->cpending = true;
  a.group_sum = ws->d_cprefix;
  a.emit_done = reinterpret_cast<uint32_t*>(ws->d_cprefix + ws->cgroups);
  a.tally = d_tally;
  a.n_fid = d_tally ? n_fid : 0;
  codon_codes(code, a.codon_codes);
  *out = a;
  return KMA_OK;
}

// Canonical-order emission after the probe on s (whose atomics summed the block counts into
// ws's group sums); the emit pass leaves the sums zero for the next call.
int enqueue_contig_emit(kma_workspace* ws, kma::ContigArgs a, kma_hit* d_hits, uint64_t cap,
                        uint64_t* d_n_hits, hipStream_t s) {
  const uint64_t nb = contig_blocks(a.total_bases);
  a.out = d_hits;
  a.cap = d_hits ? cap : 0;
  a.n_hits = d_n_hits;
  KMA_HIP(kma::launch_contigs_emit(a, nb, s));
  ws->cpending = false;
  return KMA_OK;
}

// One shard [lo, hi) of a host 6-frame call on replica r. out_hits == null: count the shard's
// hits into *n_hits and accumulate the tally rows of its contigs (tally = the caller's rows
// lo..hi); else emit the *n_hits hits (contig indices relative to lo) into *out_hits.
// strict: the KmerFactory.Strict two-pass form of the peg join (single replica).
int contig_shard(kma_table* t, const Replica& r, const uint8_t* dna, const uint64_t* offsets,
                 uint32_t lo, uint32_t hi, int genetic_code, bool strict,
                 std::vector<kma_hit>* out_hits, uint64_t* n_hits, uint32_t* tally,
                 uint32_t n_fid) {
  const uint32_t n = hi - lo;
  const uint64_t base = offsets[lo], total = offsets[hi] - base;
  if (!out_hits) *n_hits = 0;
  if (n == 0 || total == 0) return KMA_OK;
  const char* code = ncbi_code(genetic_code);
  HostCtx* c = nullptr;
  if (int rc = acquire_ctx(t, r.device, &c)) return rc;
  CtxGuard guard{t, c};
  DeviceScope ds(r.device);
  if (ds.err != hipSuccess) return fail(KMA_E_DEVICE, "hipSetDevice(%d)", r.device);
  if (int rc = kma_workspace_reserve_contigs(c->ws, total)) return rc;
  const size_t in_bytes = (total + 64 + 7) & ~7ull, off_bytes = (n + 1) * 8ull;
  const size_t tb = tally ? (size_t)n * n_fid * 4 : 0;
  KMA_HIP(c->d_in.reserve(in_bytes));
  KMA_HIP(c->d_off.reserve(n + 1));
  KMA_HIP(c->h_in.reserve(in_bytes + off_bytes + tb));
  uint8_t* hin = c->h_in.p;
  hipStream_t s = c->stream;
  KMA_HIP(stage_h2d(c->d_in.p, hin, dna + base, total, s));
  std::memset(hin + total, 0, in_bytes - total);
  KMA_HIP(hipMemcpyAsync(c->d_in.p + total, hin + total, in_bytes - total,
                         hipMemcpyHostToDevice, s));
  uint64_t* hoff = reinterpret_cast<uint64_t*>(hin + in_bytes);
  for (uint32_t i = 0; i <= n; ++i) hoff[i] = offsets[lo + i] - base;
  KMA_HIP(hipMemcpyAsync(c->d_off.p, hoff, off_bytes, hipMemcpyHostToDevice, s));
  // d_out: [n_hits u64, pad | tally]; slot counts (strict) in d_aux; hits in d_hits.
  KMA_HIP(c->d_out.reserve(16 + tb));
  uint64_t* d_n = reinterpret_cast<uint64_t*>(c->d_out.p);
  uint32_t* d_tally = tally ? reinterpret_cast<uint32_t*>(c->d_out.p + 16) : nullptr;
  if (tb) {
    uint8_t* ht = hin + in_bytes + off_bytes;
    std::memcpy(ht, tally, tb);
    KMA_HIP(hipMemcpyAsync(d_tally, ht, tb, hipMemcpyHostToDevice, s));
  }
  kma::ContigArgs a;
  if (int rc = contig_args(t, r, c->ws, c->d_in.p, c->d_off.p, n, total, code, d_tally, n_fid, s,
                           &a))
    return rc;
  const uint64_t nb = contig_blocks(total);
  if (strict) {
    const uint64_t n_slots = t->n_buckets * kma::slots_for_k(t->k);
    KMA_HIP(c->d_aux.reserve(n_slots));
    KMA_HIP(hipMemsetAsync(c->d_aux.p, 0, n_slots * 4, s));
    a.slot_count = c->d_aux.p;
    a.strict_pass = 1;  // count every table key's locations
    uint64_t* const gs = a.group_sum;
    a.group_sum = nullptr;  // no emit follows this pass
    KMA_HIP(kma::launch_contigs_probe(a, nb, s));
    a.group_sum = gs;
    a.strict_pass = 2;  // keep keys with exactly one location
  }
  KMA_HIP(kma::launch_contigs_probe(a, nb, s));
  if (!out_hits) {  // pass 1: count (and tally)
    if (int rc = enqueue_contig_emit(c->ws, a, nullptr, 0, d_n, s)) return rc;
    KMA_HIP(c->h_out.reserve(16 + tb));
    KMA_HIP(hipMemcpyAsync(c->h_out.p, d_n, 8, hipMemcpyDeviceToHost, s));
    if (tb) KMA_HIP(hipMemcpyAsync(c->h_out.p + 16, d_tally, tb, hipMemcpyDeviceToHost, s));
    KMA_HIP(hipStreamSynchronize(s));
    std::memcpy(n_hits, c->h_out.p, 8);
    if (tb) std::memcpy(tally, c->h_out.p + 16, tb);
    return KMA_OK;
  }
  // pass 2: emit into d_hits (sized by pass 1's count, passed in *n_hits)
  const uint64_t cap = *n_hits;
  KMA_HIP(c->d_hits.reserve(std::max<uint64_t>(cap, 1)));
  if (int rc = enqueue_contig_emit(c->ws, a, c->d_hits.p, cap, d_n, s)) return rc;
  KMA_HIP(c->h_out.reserve(16 + cap * sizeof(kma_hit)));
  KMA_HIP(hipMemcpyAsync(c->h_out.p, d_n, 8, hipMemcpyDeviceToHost, s));
  KMA_HIP(hipMemcpyAsync(c->h_out.p + 16, c->d_hits.p, cap * sizeof(kma_hit),
                         hipMemcpyDeviceToHost, s));
  KMA_HIP(hipStreamSynchronize(s));
  uint64_t nh = 0;
  std::memcpy(&nh, c->h_out.p, 8);
  if (nh != cap) return fail(KMA_E_DEVICE, "6-frame pass: %llu hits, then %llu",
                             (unsigned long long)cap, (unsigned long long)nh);
  out_hits->resize(nh);
  std::memcpy(out_hits->data(), c->h_out.p + 16, nh * sizeof(kma_hit));
  return KMA_OK;
}

int annotate_contigs_host(kma_table* t, const uint8_t* dna, const uint64_t* offsets,
                          uint32_t n_contig, int genetic_code, bool strict, kma_hit* out_hits,
                          uint64_t cap, uint64_t* n_hits, uint32_t* out_tally, uint32_t n_fid) {
  if (!t || !n_hits) return fail(KMA_E_INVALID, "null argument");
  if (!ncbi_code(genetic_code))
    return fail(KMA_E_INVALID, "unsupported genetic code %d", genetic_code);
  *n_hits = 0;
  if (n_contig == 0) return KMA_OK;
  if (!dna || !offsets) return fail(KMA_E_INVALID, "null argument");
  for (uint32_t c = 0; c < n_contig; ++c)
    if (offsets[c + 1] < offsets[c]) return fail(KMA_E_INVALID, "offsets decrease at %u", c);
  if (offsets[n_contig] - offsets[0] >= (1ull << 39))
    return fail(KMA_E_INVALID, "more than 2^39 bases in one call");
  const bool tally = out_tally && n_fid;
  const std::vector<Replica> reps = replicas(t);
  const int nr = strict ? 1 : (int)std::min<uint64_t>(reps.size(), n_contig);
  const std::vector<uint32_t> b = shard_bounds(offsets, n_contig, nr);
  // Pass 1 counts (and tallies into copies: nothing is written on KMA_E_CAPACITY); pass 2
  // emits. A shard's hits are produced only if the whole call fits in cap.
  std::vector<uint64_t> nh(nr, 0);
  std::vector<std::vector<uint32_t>> tal(tally ? nr : 0);
  for (int i = 0; i < (tally ? nr : 0); ++i)
    tal[i].assign(out_tally + (uint64_t)b[i] * n_fid, out_tally + (uint64_t)b[i + 1] * n_fid);
  const size_t width = staging_width(nr);
  int rc = fan_out(nr, [&](int i) {
    ShardWidth sw(width);
    return contig_shard(t, reps[i], dna, offsets, b[i], b[i + 1], genetic_code, strict,
                        nullptr, &nh[i], tally ? tal[i].data() : nullptr, n_fid);
  });
  if (rc != KMA_OK) return rc;
  uint64_t total = 0;
  for (uint64_t x : nh) total += x;
  *n_hits = total;
  if (total > cap || (total && !out_hits))
    return fail(KMA_E_CAPACITY, "%llu hits, capacity %llu", (unsigned long long)total,
                (unsigned long long)(out_hits ? cap : 0));
  for (int i = 0; i < (tally ? nr : 0); ++i)
    std::copy(tal[i].begin(), tal[i].end(), out_tally + (uint64_t)b[i] * n_fid);
  if (total == 0) return KMA_OK;
  std::vector<std::vector<kma_hit>> hv(nr);
  rc = fan_out(nr, [&](int i) {
    ShardWidth sw(width);
    if (nh[i] == 0) return KMA_OK;
    return contig_shard(t, reps[i], dna, offsets, b[i], b[i + 1], genetic_code, strict,
                        &hv[i], &nh[i], nullptr, 0);
  });
  if (rc != KMA_OK) return rc;
  uint64_t o = 0;
  for (int i = 0; i < nr; ++i)
    for (const kma_hit& h : hv[i]) {
      out_hits[o] = h;
      out_hits[o++].contig += b[i];
    }
  return KMA_OK;
}
}  // namespace

extern "C" {

int kma_workspace_reserve_contigs(kma_workspace* ws, uint64_t n_bases) {
  if (!ws) return fail(KMA_E_INVALID, "null workspace");
  if (n_bases >= (1ull << 39)) return fail(KMA_E_INVALID, "more than 2^39 bases in one call");
  if (ws->d_cstage && n_bases <= ws->contig_cap) return KMA_OK;
  DeviceScope ds(ws->device);
  if (ds.err != hipSuccess) return fail(KMA_E_DEVICE, "hipSetDevice(%d)", ws->device);
  free_contig_scratch(ws);
  const uint64_t nb = contig_blocks(n_bases);
  const uint64_t ng = (nb + kma::kScanGroup - 1) / kma::kScanGroup;
  KMA_HIP(hipMalloc(&ws->d_cstage, nb * 2 * kma::kContigTile * sizeof(kma_hit)));
  KMA_HIP(hipMalloc(&ws->d_ccounts, ng * kma::kScanGroup * 4));
  KMA_HIP(hipMalloc(&ws->d_cprefix, (ng + 1) * 8));
  KMA_HIP(hipMemset(ws->d_cprefix, 0, (ng + 1) * 8));
  ws->cgroups = ng;
  ws->cpending = false;
  ws->contig_cap = nb * kma::kContigTile;
  return KMA_OK;
}

uint64_t kma_contig_window_count(const uint64_t* offsets, uint32_t n_contig, int k) {
  uint64_t n = 0;
  for (uint32_t c = 0; c < n_contig; ++c) {
    const int64_t len = (int64_t)(offsets[c + 1] - offsets[c]);
    const int64_t per = len - 3 * k - 2;  // sum over frames of max(0, P_f - K), per strand
    if (per > 0) n += 2 * (uint64_t)per;
  }
  return n;
}

int kma_annotate_contigs_device(const kma_table* t, kma_workspace* ws, const uint8_t* d_dna,
                                const uint64_t* d_offsets, uint32_t n_contig, uint64_t n_bases,
                                int genetic_code, kma_hit* d_hits, uint64_t cap,
                                uint64_t* d_n_hits, uint32_t* d_tally, uint32_t n_fid,
                                void* stream) {
  if (!t || !ws) return fail(KMA_E_INVALID, "null table or workspace");
  Replica rep;
  if (!replica_on(t, ws->device, &rep))
    return fail(KMA_E_INVALID, "table has no replica on the workspace's device %d", ws->device);
  const Replica* r = &rep;
  const char* code = ncbi_code(genetic_code);
  if (!code) return fail(KMA_E_INVALID, "unsupported genetic code %d", genetic_code);
  if (!d_n_hits) return fail(KMA_E_INVALID, "null n_hits");
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceScope ds(r->device);
  if (ds.err != hipSuccess) return fail(KMA_E_DEVICE, "hipSetDevice(%d)", r->device);
  if (n_contig == 0 || n_bases == 0) {
    KMA_HIP(hipMemsetAsync(d_n_hits, 0, 8, s));
    return KMA_OK;
  }
  if (!d_dna || !d_offsets) return fail(KMA_E_INVALID, "null device buffer");
  if (n_bases > ws->contig_cap)
    return fail(KMA_E_CAPACITY, "workspace reserved for %llu bases, call needs %llu",
                (unsigned long long)ws->contig_cap, (unsigned long long)n_bases);
  kma::ContigArgs a;
  if (int rc = contig_args(t, *r, ws, d_dna, d_offsets, n_contig, n_bases, code, d_tally, n_fid,
                           s, &a))
    return rc;
  PhaseClock clk(ws, s, kContigPhases, 2);
  KMA_HIP(clk.mark());
  const uint64_t nb = contig_blocks(n_bases);
  KMA_HIP(kma::launch_contigs_probe(a, nb, s));
  KMA_HIP(clk.mark());
  const int rc = enqueue_contig_emit(ws, a, d_hits, cap, d_n_hits, s);
  if (rc == KMA_OK) KMA_HIP(clk.mark());
  return rc;
}

int kma_annotate_contigs(const kma_table* t, const uint8_t* dna, const uint64_t* offsets,
                         uint32_t n_contig, int genetic_code, kma_hit* out_hits, uint64_t cap,
                         uint64_t* n_hits, uint32_t* out_tally, uint32_t n_fid) {
  return annotate_contigs_host(const_cast<kma_table*>(t), dna, offsets, n_contig, genetic_code,
                               false, out_hits, cap, n_hits, out_tally, n_fid);
}

int kma_connect_pegs(const kma_table* t, const uint8_t* dna, const uint64_t* offsets,
                     uint32_t n_contig, int genetic_code, int strict, kma_hit* out_hits,
                     uint64_t cap, uint64_t* n_hits) {
  return annotate_contigs_host(const_cast<kma_table*>(t), dna, offsets, n_contig, genetic_code,
                               strict != 0, out_hits, cap, n_hits, nullptr, 0);
}

}  // extern "C"
