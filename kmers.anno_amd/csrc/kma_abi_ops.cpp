// kma_abi_ops.cpp — the projector's one-shot operators of the C ABI (include/kmeranno.h) that
// build no ProteinKmers sets (those are in kma_abi_sets.cpp): peg table, signatures, peg
// proposals, ORF index, translation and the sequence MD5 / duplicate check. Each checks its
// arguments on the host, enters its device, stages its batch in buffers of its own (kma_host.h:
// upload_batch, Scratch, AlphabetFlag), runs its launchers (kma_build.hip, kma_proposals.hip,
// kma_orf.hip, kma_translate.hip, kma_md5.hip) on the null stream and copies the results back.
// The streamed signature build (kma_sig_builder, kma_sigmerge.hip) is here too: an object that
// keeps its run and its scratch between calls.
#include <memory>

#include "kma_internal.h"
#include "kma_md5.h"
#include "kma_objects.h"
#include "kma_orf.h"
#include "kma_sigmerge.h"
#include "kma_translate.h"

using namespace kma::host;

extern "C" {

int kma_peg_table_create(const uint8_t* residues, const uint64_t* offsets, uint32_t n_peg, int k,
                         int device, double load_factor, kma_table** out,
                         uint64_t* n_windows) {
  if (!out) return fail(KMA_E_INVALID, "null argument");
  *out = nullptr;
  if (int rc = check_k(k)) return rc;
  if (load_factor <= 0) load_factor = 0.5;
  if (load_factor > 0.95) return fail(KMA_E_INVALID, "load factor %.3f > 0.95", load_factor);
  if (n_peg > KMA_MAX_FID + 1u) return fail(KMA_E_INVALID, "more than 2^22 pegs");
  if (n_peg && (!residues || !offsets)) return fail(KMA_E_INVALID, "null argument");
  if (int rc = check_offsets(offsets, n_peg, "", 0, nullptr)) return rc;
  const uint64_t total = n_peg ? offsets[n_peg] - offsets[0] : 0;
  uint8_t lut[256];
  standard_lut(lut);
  DeviceScope ds(device);
  if (int rc = ds.entered()) return rc;
  DevBufs b;
  uint8_t *d_lut, *d_flags;
  uint64_t *d_keys, *d_keys2, *d_n;
  uint32_t *d_pegs, *d_pegs2;
  const uint64_t nw = std::max<uint64_t>(total, 1);
  KMA_HIP(b.alloc(&d_lut, 256));
  KMA_HIP(b.alloc(&d_keys, nw * 8));
  KMA_HIP(b.alloc(&d_keys2, nw * 8));
  KMA_HIP(b.alloc(&d_pegs, nw * 4));
  KMA_HIP(b.alloc(&d_pegs2, nw * 4));
  KMA_HIP(b.alloc(&d_flags, nw));
  KMA_HIP(b.alloc(&d_n, 8));
  KMA_HIP(hipMemset(d_n, 0, 8));
  uint64_t n_sel = 0, windows = 0;
  if (total) {  // (an empty batch stages nothing: the table is built from no keys)
    for (uint32_t s = 0; s < n_peg; ++s) {
      const uint64_t L = offsets[s + 1] - offsets[s];
      if (L > (uint64_t)k) windows += L - k;
    }
    DevBatch in;
    if (int rc = upload_batch(b, residues, offsets, n_peg, 64, &in)) return rc;
    KMA_HIP(hipMemcpy(d_lut, lut, 256, hipMemcpyHostToDevice));
    KMA_HIP(kma::launch_peg_windows(in.bytes, in.off, n_peg, k, d_lut, d_keys, d_pegs, nullptr));
    Scratch tmp;
    KMA_HIP(kma::launch_sort_pairs(nullptr, tmp.ask(), d_keys, d_keys2, d_pegs, d_pegs2, total,
                                   5 * k, nullptr));
    KMA_HIP(kma::launch_select_flagged(nullptr, tmp.ask(), d_keys2, d_pegs2, d_flags, d_keys,
                                       d_pegs, d_n, total, nullptr));
    KMA_HIP(tmp.alloc(b));
    KMA_HIP(kma::launch_sort_pairs(tmp.p, tmp.bytes(), d_keys, d_keys2, d_pegs, d_pegs2, total,
                                   5 * k, nullptr));
    KMA_HIP(kma::launch_singleton_flags(d_keys2, total, d_flags, nullptr));
    KMA_HIP(kma::launch_select_flagged(tmp.p, tmp.bytes(), d_keys2, d_pegs2, d_flags, d_keys,
                                       d_pegs, d_n, total, nullptr));
    KMA_HIP(hipMemcpy(&n_sel, d_n, 8, hipMemcpyDeviceToHost));
  }
  if (n_windows) *n_windows = windows;
  const int rc = create_from_device_keys(d_keys, d_pegs, n_sel, k, device, load_factor, lut, out);
  if (rc != KMA_OK) return rc;
  (*out)->info.n_rows = windows;
  return KMA_OK;
}

int kma_build_signatures(const uint8_t* residues, const uint64_t* offsets, const int32_t* roles,
                         uint32_t n_seq, int k, uint32_t flags, int device, uint64_t* out_keys,
                         uint32_t* out_roles, uint64_t cap, uint64_t* n_out) {
  if (!n_out) return fail(KMA_E_INVALID, "null argument");
  *n_out = 0;
  if (int rc = check_k(k)) return rc;
  if (flags & ~KMA_F_END_EXCLUSIVE) return fail(KMA_E_INVALID, "bad flags");
  if (n_seq == 0) return KMA_OK;
  if (!residues || !offsets || !roles) return fail(KMA_E_INVALID, "null argument");
  // (not check_offsets: a protein's role is checked on the way, before a later decrease)
  for (uint32_t s = 0; s < n_seq; ++s) {
    if (offsets[s + 1] < offsets[s]) return fail(KMA_E_INVALID, "offsets decrease at %u", s);
    if (roles[s] >= (int32_t)kma::kBuildNeg)
      return fail(KMA_E_INVALID, "role %d of protein %u >= 2^24 - 1", roles[s], s);
  }
  const uint64_t total = offsets[n_seq] - offsets[0];
  if (total == 0) return KMA_OK;
  if (total >= (1ull << 31)) return fail(KMA_E_INVALID, "more than 2^31 residues in one call");
  uint8_t lut[256];
  standard_lut(lut);
  DeviceScope ds(device);
  if (int rc = ds.entered()) return rc;
  DevBufs b;
  DevBatch in;
  if (int rc = upload_batch(b, residues, offsets, n_seq, 64, &in)) return rc;
  uint8_t *d_lut, *d_flags;
  uint64_t *d_ka, *d_kb, *d_n;
  int32_t* d_roles;
  uint32_t *d_ta, *d_tb, *d_head, *d_run;
  KMA_HIP(b.alloc(&d_roles, n_seq * 4ull));
  KMA_HIP(b.alloc(&d_lut, 256));
  KMA_HIP(b.alloc(&d_ka, total * 8));
  KMA_HIP(b.alloc(&d_kb, total * 8));
  KMA_HIP(b.alloc(&d_ta, total * 4));
  KMA_HIP(b.alloc(&d_tb, total * 4));
  KMA_HIP(b.alloc(&d_head, total * 4));
  KMA_HIP(b.alloc(&d_run, total * 4));
  KMA_HIP(b.alloc(&d_flags, total));
  KMA_HIP(b.alloc(&d_n, 16));
  KMA_HIP(hipMemcpy(d_roles, roles, n_seq * 4ull, hipMemcpyHostToDevice));
  KMA_HIP(hipMemcpy(d_lut, lut, 256, hipMemcpyHostToDevice));
  AlphabetFlag alpha;
  if (int rc = alpha.init(b)) return rc;
  KMA_HIP(kma::launch_build_windows(in.bytes, in.off, n_seq, d_roles, k,
                                    (flags & KMA_F_END_EXCLUSIVE) ? 1 : 0, d_lut, d_ka, d_ta,
                                    alpha.d, nullptr));
  // (key, role) pairs sorted by key; RoleCounter per key run; select the good runs' heads
  Scratch tmp;
  KMA_HIP(kma::launch_sort_pairs(nullptr, tmp.ask(), d_ka, d_kb, d_ta, d_tb, total, 5 * k,
                                 nullptr));
  KMA_HIP(kma::launch_signature_flags(d_kb, d_tb, total, d_flags, d_head, d_run, nullptr,
                                      tmp.ask(), nullptr));
  KMA_HIP(kma::launch_select_flagged(nullptr, tmp.ask(), d_kb, d_tb, d_flags, d_ka, d_ta, d_n,
                                     total, nullptr));
  KMA_HIP(tmp.alloc(b));
  KMA_HIP(kma::launch_sort_pairs(tmp.p, tmp.bytes(), d_ka, d_kb, d_ta, d_tb, total, 5 * k,
                                 nullptr));
  KMA_HIP(kma::launch_signature_flags(d_kb, d_tb, total, d_flags, d_head, d_run, tmp.p,
                                      tmp.bytes(), nullptr));
  KMA_HIP(kma::launch_select_flagged(tmp.p, tmp.bytes(), d_kb, d_tb, d_flags, d_ka, d_ta, d_n,
                                     total, nullptr));
  uint64_t n_sel = 0;
  KMA_HIP(hipMemcpy(&n_sel, d_n, 8, hipMemcpyDeviceToHost));
  if (int rc = alpha.check()) return rc;
  *n_out = n_sel;
  if (n_sel > cap || (n_sel && (!out_keys || !out_roles)))
    return fail(KMA_E_CAPACITY, "%llu signature kmers, capacity %llu",
                (unsigned long long)n_sel, (unsigned long long)cap);
  if (n_sel == 0) return KMA_OK;
  KMA_HIP(hipMemcpy(out_keys, d_ka, n_sel * 8, hipMemcpyDeviceToHost));
  KMA_HIP(hipMemcpy(out_roles, d_ta, n_sel * 4, hipMemcpyDeviceToHost));
  return KMA_OK;
}

}  // extern "C"

// ---- streamed signature build (kma_sigmerge.hip) ------------------------------------------------
// The builder's small device block: the LUT, then the words a call reads back.
namespace {
constexpr size_t kSigAlpha = 256, kSigNB = 264, kSigCounts = 272, kSigSmall = 304;

uint64_t sig_builder_bytes(const kma_sig_builder* b) {
  uint64_t n = kSigSmall;
  for (int i = 0; i < 2; ++i) n += b->run_keys[i].cap * 8 + b->run_states[i].cap * 4;
  n += b->in.cap + b->off.cap * 8 + b->roles.cap * 4 + (b->ka.cap + b->kb.cap) * 8;
  n += (b->ta.cap + b->tb.cap + b->head.cap + b->run.cap) * 4 + b->hflags.cap;
  return n + b->tiles.cap * 8 + b->temp.cap;
}
}  // namespace

extern "C" {

int kma_sig_builder_create(int k, uint32_t flags, int device, kma_sig_builder** out) {
  if (!out) return fail(KMA_E_INVALID, "null argument");
  *out = nullptr;
  if (int rc = check_k(k)) return rc;
  if (flags & ~KMA_F_END_EXCLUSIVE) return fail(KMA_E_INVALID, "bad flags");
  uint8_t lut[256];
  standard_lut(lut);
  DeviceScope ds(device);
  if (int rc = ds.entered()) return rc;
  std::unique_ptr<kma_sig_builder> b(new kma_sig_builder);
  b->device = device;
  b->k = k;
  b->flags = flags;
  KMA_HIP(hipMalloc(reinterpret_cast<void**>(&b->d_small), kSigSmall));
  KMA_HIP(hipMemset(b->d_small, 0, kSigSmall));
  KMA_HIP(hipMemcpy(b->d_small, lut, 256, hipMemcpyHostToDevice));
  for (hipEvent_t& e : b->ev) KMA_HIP(hipEventCreate(&e));
  *out = b.release();
  return KMA_OK;
}

int kma_sig_builder_destroy(kma_sig_builder* b) {
  if (!b) return KMA_OK;
  DeviceScope ds(b->device);
  delete b;
  return KMA_OK;
}

int kma_sig_builder_info_get(const kma_sig_builder* b, struct kma_sig_builder_info* out) {
  if (!b || !out) return fail(KMA_E_INVALID, "null argument");
  out->k = b->k;
  out->flags = b->flags;
  out->tile = kma::kSigTile;
  out->n_adds = b->n_adds;
  out->n_residues = b->n_residues;
  out->n_keys = b->n_keys;
  out->n_role = b->counts[0];
  out->n_conflict = b->counts[1];
  out->n_buffered = b->counts[2];
  out->bytes = sig_builder_bytes(b);
  return KMA_OK;
}

int kma_sig_builder_add(kma_sig_builder* b, const uint8_t* residues, const uint64_t* offsets,
                        const int32_t* roles, uint32_t n_seq) {
  if (!b) return fail(KMA_E_INVALID, "null argument");
  if (n_seq == 0) return ++b->n_adds, KMA_OK;
  if (!residues || !offsets || !roles) return fail(KMA_E_INVALID, "null argument");
  for (uint32_t s = 0; s < n_seq; ++s) {
    if (offsets[s + 1] < offsets[s]) return fail(KMA_E_INVALID, "offsets decrease at %u", s);
    if (roles[s] >= (int32_t)kma::kBuildNeg)
      return fail(KMA_E_INVALID, "role %d of protein %u >= 2^24 - 1", roles[s], s);
  }
  const uint64_t total = offsets[n_seq] - offsets[0];
  if (total == 0) return ++b->n_adds, KMA_OK;
  if (total >= (1ull << 31)) return fail(KMA_E_INVALID, "more than 2^31 residues in one add");
  DeviceScope ds(b->device);
  if (int rc = ds.entered()) return rc;
  // the batch scratch (nothing of the resident run is touched before the swap at the end)
  constexpr uint64_t kPad = 64;
  KMA_HIP(b->in.reserve(total + kPad));
  KMA_HIP(b->off.reserve(n_seq + 1ull));
  KMA_HIP(b->roles.reserve(n_seq));
  KMA_HIP(b->ka.reserve(total));
  KMA_HIP(b->kb.reserve(total));
  KMA_HIP(b->ta.reserve(total));
  KMA_HIP(b->tb.reserve(total));
  KMA_HIP(b->head.reserve(total));
  KMA_HIP(b->run.reserve(total));
  KMA_HIP(b->hflags.reserve(total));
  uint64_t* const d_nb = reinterpret_cast<uint64_t*>(b->d_small + kSigNB);
  uint32_t* const d_alpha = reinterpret_cast<uint32_t*>(b->d_small + kSigAlpha);
  unsigned long long* const d_counts =
      reinterpret_cast<unsigned long long*>(b->d_small + kSigCounts);
  const int bits = 5 * b->k;
  size_t need = 0, q = 0;
  KMA_HIP(kma::launch_sort_pairs(nullptr, &q, b->ka.p, b->kb.p, b->ta.p, b->tb.p, total, bits,
                                 nullptr));
  need = std::max(need, q);
  KMA_HIP(kma::launch_sig_reduce(b->kb.p, b->tb.p, total, b->hflags.p, b->head.p, b->run.p,
                                 b->ka.p, b->ta.p, d_nb, nullptr, &q, nullptr));
  need = std::max(need, q);
  KMA_HIP(b->temp.reserve(need));
  // stage, windows, sort, reduce
  {
    std::vector<uint64_t> rel(n_seq + 1ull);
    rebase_offsets(rel.data(), offsets, n_seq + 1ull, offsets[0]);
    KMA_HIP(hipMemcpy(b->in.p, residues + offsets[0], total, hipMemcpyHostToDevice));
    KMA_HIP(hipMemset(b->in.p + total, 0, kPad));
    KMA_HIP(hipMemcpy(b->off.p, rel.data(), (n_seq + 1ull) * 8, hipMemcpyHostToDevice));
    KMA_HIP(hipMemcpy(b->roles.p, roles, n_seq * 4ull, hipMemcpyHostToDevice));
  }
  KMA_HIP(hipMemset(d_alpha, 0, 4));
  KMA_HIP(hipMemset(d_nb, 0, 8));
  KMA_HIP(hipEventRecord(b->ev[0], nullptr));
  KMA_HIP(kma::launch_build_windows(b->in.p, b->off.p, n_seq, b->roles.p, b->k,
                                    (b->flags & KMA_F_END_EXCLUSIVE) ? 1 : 0, b->d_small, b->ka.p,
                                    b->ta.p, d_alpha, nullptr));
  KMA_HIP(hipEventRecord(b->ev[1], nullptr));
  q = b->temp.cap;
  KMA_HIP(kma::launch_sort_pairs(b->temp.p, &q, b->ka.p, b->kb.p, b->ta.p, b->tb.p, total, bits,
                                 nullptr));
  KMA_HIP(hipEventRecord(b->ev[2], nullptr));
  q = b->temp.cap;
  KMA_HIP(kma::launch_sig_reduce(b->kb.p, b->tb.p, total, b->hflags.p, b->head.p, b->run.p,
                                 b->ka.p, b->ta.p, d_nb, b->temp.p, &q, nullptr));
  KMA_HIP(hipEventRecord(b->ev[3], nullptr));
  uint64_t n_b = 0;
  uint32_t alpha = 0;
  KMA_HIP(hipMemcpy(&n_b, d_nb, 8, hipMemcpyDeviceToHost));
  KMA_HIP(hipMemcpy(&alpha, d_alpha, 4, hipMemcpyDeviceToHost));
  if (alpha) return fail(KMA_E_ALPHABET, "a protein window holds a byte outside A-Z and '*'");
  if (n_b == 0) {  // no counted window
    ++b->n_adds;
    b->n_residues += total;
    return KMA_OK;
  }
  // union merge of the resident run with the reduced batch into the other run buffer
  const kma::SigRun ra{b->run_keys[b->cur].p, b->run_states[b->cur].p, b->n_keys};
  const kma::SigRun rb{b->ka.p, b->ta.p, n_b};
  const uint64_t n_tiles = kma::sig_tiles(ra.n, rb.n, kma::kSigTile);
  KMA_HIP(b->tiles.reserve(2 * (n_tiles + 1)));
  uint64_t* const tile_cnt = b->tiles.p;
  uint64_t* const tile_off = b->tiles.p + n_tiles + 1;
  KMA_HIP(kma::launch_sig_merge_count(ra, rb, tile_cnt, tile_off, nullptr, &q, nullptr));
  KMA_HIP(b->temp.reserve(q));
  q = b->temp.cap;
  KMA_HIP(hipEventRecord(b->ev[4], nullptr));
  KMA_HIP(kma::launch_sig_merge_count(ra, rb, tile_cnt, tile_off, b->temp.p, &q, nullptr));
  KMA_HIP(hipEventRecord(b->ev[5], nullptr));
  uint64_t n_out = 0;
  KMA_HIP(hipMemcpy(&n_out, tile_off + n_tiles, 8, hipMemcpyDeviceToHost));
  if (n_out >= (1ull << 32))
    return fail(KMA_E_CAPACITY, "%llu resident keys: a builder holds fewer than 2^32",
                (unsigned long long)n_out);
  const int nxt = b->cur ^ 1;
  KMA_HIP(b->run_keys[nxt].reserve(n_out));
  KMA_HIP(b->run_states[nxt].reserve(n_out));
  KMA_HIP(hipMemset(d_counts, 0, 24));
  KMA_HIP(hipEventRecord(b->ev[6], nullptr));
  KMA_HIP(kma::launch_sig_merge_write(ra, rb, tile_off, b->run_keys[nxt].p, b->run_states[nxt].p,
                                      nullptr));
  KMA_HIP(hipEventRecord(b->ev[7], nullptr));
  KMA_HIP(kma::launch_sig_counts(b->run_states[nxt].p, n_out, d_counts, nullptr));
  KMA_HIP(hipEventRecord(b->ev[8], nullptr));
  uint64_t counts[3];
  KMA_HIP(hipMemcpy(counts, d_counts, 24, hipMemcpyDeviceToHost));
  const int first_event[6] = {0, 1, 2, 4, 6, 7};  // a stage runs from its event to the next one
  for (int i = 0; i < 6; ++i) {
    float ms = 0.f;
    KMA_HIP(hipEventElapsedTime(&ms, b->ev[first_event[i]], b->ev[first_event[i] + 1]));
    b->stage_ms[i] = ms;
  }
  b->cur = nxt;
  b->n_keys = n_out;
  std::copy(counts, counts + 3, b->counts);
  ++b->n_adds;
  b->n_residues += total;
  return KMA_OK;
}

// Not in kmeranno.h: measurement hook (scripts/sigbuild_rate.py). hipEvent times of the stages of
// the builder's last add that merged: windows, sort, reduce, the merge's count pass with its
// scan, its write pass, the counts.
int kma_debug_sig_builder_ms(const kma_sig_builder* b, double* out6) {
  if (!b || !out6) return fail(KMA_E_INVALID, "null argument");
  std::copy(b->stage_ms, b->stage_ms + 6, out6);
  return KMA_OK;
}

int kma_sig_builder_finish(const kma_sig_builder* b, uint64_t* out_keys, uint32_t* out_roles,
                           uint64_t cap, uint64_t* n_out) {
  if (!b || !n_out) return fail(KMA_E_INVALID, "null argument");
  const uint64_t n_sel = b->counts[0];
  *n_out = n_sel;
  if (n_sel > cap || (n_sel && (!out_keys || !out_roles)))
    return fail(KMA_E_CAPACITY, "%llu signature kmers, capacity %llu",
                (unsigned long long)n_sel, (unsigned long long)cap);
  if (n_sel == 0) return KMA_OK;
  DeviceScope ds(b->device);
  if (int rc = ds.entered()) return rc;
  // buffers of the call's own: the builder is left as it is
  DevBufs bufs;
  uint8_t* d_flags;
  uint64_t *d_keys, *d_n;
  uint32_t* d_roles;
  KMA_HIP(bufs.alloc(&d_flags, b->n_keys));
  KMA_HIP(bufs.alloc(&d_keys, n_sel * 8));
  KMA_HIP(bufs.alloc(&d_roles, n_sel * 4));
  KMA_HIP(bufs.alloc(&d_n, 8));
  const uint64_t* keys = b->run_keys[b->cur].p;
  const uint32_t* states = b->run_states[b->cur].p;
  Scratch tmp;
  KMA_HIP(kma::launch_select_flagged(nullptr, tmp.ask(), keys, states, d_flags, d_keys, d_roles,
                                     d_n, b->n_keys, nullptr));
  KMA_HIP(tmp.alloc(bufs));
  KMA_HIP(kma::launch_sig_role_flags(states, b->n_keys, d_flags, nullptr));
  KMA_HIP(kma::launch_select_flagged(tmp.p, tmp.bytes(), keys, states, d_flags, d_keys, d_roles,
                                     d_n, b->n_keys, nullptr));
  uint64_t got = 0;
  KMA_HIP(hipMemcpy(&got, d_n, 8, hipMemcpyDeviceToHost));
  if (got != n_sel)
    return fail(KMA_E_DEVICE, "%llu rows selected, %llu counted", (unsigned long long)got,
                (unsigned long long)n_sel);
  KMA_HIP(hipMemcpy(out_keys, d_keys, n_sel * 8, hipMemcpyDeviceToHost));
  KMA_HIP(hipMemcpy(out_roles, d_roles, n_sel * 4, hipMemcpyDeviceToHost));
  return KMA_OK;
}

}  // extern "C"

extern "C" {

int kma_propose_pegs(const kma_hit* hits, uint64_t n_hits, const uint32_t* peg_len,
                     uint32_t n_peg, int k, double min_strength, double max_fuzz,
                     double min_fuzz, int device, kma_proposal* out, uint64_t cap,
                     uint64_t* n_out, uint64_t* stats) {
  if (!n_out || !stats) return fail(KMA_E_INVALID, "null argument");
  if (int rc = check_k(k)) return rc;
  *n_out = 0;
  stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (n_hits == 0) return KMA_OK;
  if (!hits || !peg_len || n_peg == 0) return fail(KMA_E_INVALID, "null argument");
  if (cap && !out) return fail(KMA_E_INVALID, "null output");
  if (n_hits >= (1ull << 31)) return fail(KMA_E_INVALID, "more than 2^31 connections");
  if ((uint64_t)n_peg * 6 >= (1ull << 32)) return fail(KMA_E_INVALID, "too many pegs");
  for (uint64_t i = 0; i < n_hits; ++i) {
    const kma_hit& h = hits[i];
    if (h.fid >= n_peg) return fail(KMA_E_INVALID, "connection %llu: peg %u >= %u",
                                    (unsigned long long)i, h.fid, n_peg);
    if (h.strand != '+' && h.strand != '-')
      return fail(KMA_E_INVALID, "connection %llu: strand must be '+' or '-'",
                  (unsigned long long)i);
    if (i && (h.contig < hits[i - 1].contig ||
              (h.contig == hits[i - 1].contig && h.left < hits[i - 1].left)))
      return fail(KMA_E_INVALID, "connections are not in (contig, left) order at %llu",
                  (unsigned long long)i);
  }
  DeviceScope ds(device);
  if (int rc = ds.entered()) return rc;
  const uint64_t n = n_hits;
  DevBufs b;
  kma::PropArgs a{};
  kma_hit* d_hits;
  uint32_t* d_len;
  KMA_HIP(b.alloc(&d_hits, n * sizeof(kma_hit)));
  KMA_HIP(b.alloc(&d_len, n_peg * 4ull));
  for (uint32_t** p : {&a.keys, &a.skeys, &a.idx, &a.sidx, &a.head, &a.list_no, &a.scontig,
                       &a.keep, &a.evidence, &a.out_pos})
    KMA_HIP(b.alloc(p, n * 4));
  KMA_HIP(b.alloc(&a.starts, (n + 1) * 4));
  KMA_HIP(b.alloc(&a.sleft, n * 4));
  KMA_HIP(b.alloc(&a.best, n * 4));
  KMA_HIP(b.alloc(&a.stats, 32));
  KMA_HIP(b.alloc(&a.out, n * sizeof(kma_proposal)));
  a.hits = d_hits;
  a.n = (uint32_t)n;
  a.peg_len = d_len;
  a.n_peg = n_peg;
  a.k = k;
  a.min_strength = min_strength;
  a.max_fuzz = max_fuzz;
  a.min_fuzz = min_fuzz;
  a.cap = n;
  Scratch tmp;
  KMA_HIP(kma::launch_propose(a, nullptr, tmp.ask(), nullptr));
  KMA_HIP(tmp.alloc(b));
  KMA_HIP(hipMemcpy(d_hits, hits, n * sizeof(kma_hit), hipMemcpyHostToDevice));
  KMA_HIP(hipMemcpy(d_len, peg_len, n_peg * 4ull, hipMemcpyHostToDevice));
  KMA_HIP(hipMemset(a.stats, 0, 32));
  KMA_HIP(kma::launch_propose(a, tmp.p, tmp.bytes(), nullptr));
  KMA_HIP(hipMemcpy(stats, a.stats, 32, hipMemcpyDeviceToHost));
  *n_out = stats[3];
  const uint64_t take = std::min<uint64_t>(stats[3], cap);
  if (take) KMA_HIP(hipMemcpy(out, a.out, take * sizeof(kma_proposal), hipMemcpyDeviceToHost));
  if (stats[3] > cap)
    return fail(KMA_E_CAPACITY, "%llu proposals, capacity %llu", (unsigned long long)stats[3],
                (unsigned long long)cap);
  return KMA_OK;
}

}  // extern "C"

// ---- ORF index of the projector (kma_orf.hip) ---------------------------------------------------
// One genome's stop / start scans on one device. Immutable after creation: kma_extend_proposals
// only reads it and stages every call in buffers of its own, so calls may run concurrently.
struct kma_orf_index {
  int device = 0;
  uint32_t n_contig = 0;
  int32_t* len = nullptr;      // device: n_contig contig lengths
  uint64_t* hoff = nullptr;    // device: n_contig + 1 per-strand slot offsets
  uint32_t* stop_at = nullptr; // device: 2 hoff[n_contig] words each
  uint32_t* start_at = nullptr;
  ~kma_orf_index() {
    for (void* p : {(void*)len, (void*)hoff, (void*)stop_at, (void*)start_at})
      if (p) (void)hipFree(p);
  }
};

extern "C" {

int kma_orf_index_create(const uint8_t* dna, const uint64_t* offsets, uint32_t n_contig,
                         int genetic_code, int device, kma_orf_index** out) {
  if (!out) return fail(KMA_E_INVALID, "null argument");
  *out = nullptr;
  if (!offsets) return fail(KMA_E_INVALID, "null argument");
  if (genetic_code != 1 && genetic_code != 4 && genetic_code != 11)
    return fail(KMA_E_INVALID, "genetic code %d: the ORF index knows codes 1, 4 and 11",
                genetic_code);
  std::vector<uint64_t> off(n_contig + 1ull), hoff(n_contig + 1ull);
  std::vector<int32_t> len(n_contig);
  for (uint32_t c = 0; c < n_contig; ++c) {
    if (offsets[c + 1] < offsets[c]) return fail(KMA_E_INVALID, "offsets decrease at %u", c);
    if (offsets[c + 1] - offsets[0] >= (1ull << 31))
      return fail(KMA_E_INVALID, "2^31 bases or more");
    off[c + 1] = offsets[c + 1] - offsets[0];
    len[c] = (int32_t)(offsets[c + 1] - offsets[c]);
    hoff[c + 1] = hoff[c] + 3ull * kma::orf_frame_slots((uint32_t)len[c]);
  }
  const uint64_t total = off[n_contig], half = hoff[n_contig];
  if (total && !dna) return fail(KMA_E_INVALID, "null argument");
  DeviceScope ds(device);
  if (int rc = ds.entered()) return rc;
  std::unique_ptr<kma_orf_index> idx(new kma_orf_index);
  idx->device = device;
  idx->n_contig = n_contig;
  KMA_HIP(hipMalloc(&idx->len, std::max<size_t>(n_contig * 4ull, 4)));
  KMA_HIP(hipMalloc(&idx->hoff, (n_contig + 1ull) * 8));
  KMA_HIP(hipMalloc(&idx->stop_at, std::max<size_t>(half * 8, 4)));
  KMA_HIP(hipMalloc(&idx->start_at, std::max<size_t>(half * 8, 4)));
  DevBufs b;  // the DNA and the scans' scratch live for the build only
  DevBatch in;  // (off[] is rebased already; offsets[0] is read only when there are bases)
  if (int rc = upload_batch(b, total ? dna + offsets[0] : dna, off.data(), n_contig, 0, &in))
    return rc;
  kma::OrfBuildArgs a{};
  a.dna = in.bytes;
  a.offsets = in.off;
  a.hoff = idx->hoff;
  a.n_contig = n_contig;
  a.half = half;
  a.stops = genetic_code == 4 ? kma::kOrfStops2 : kma::kOrfStops3;
  a.stop_at = idx->stop_at;
  a.start_at = idx->start_at;
  Scratch tmp;
  KMA_HIP(kma::launch_orf_build(a, nullptr, tmp.ask(), nullptr));
  KMA_HIP(tmp.alloc(b));
  KMA_HIP(hipMemcpy(idx->hoff, hoff.data(), (n_contig + 1ull) * 8, hipMemcpyHostToDevice));
  if (n_contig) KMA_HIP(hipMemcpy(idx->len, len.data(), n_contig * 4ull, hipMemcpyHostToDevice));
  KMA_HIP(kma::launch_orf_build(a, tmp.p, tmp.bytes(), nullptr));
  KMA_HIP(hipStreamSynchronize(nullptr));
  *out = idx.release();
  return KMA_OK;
}

int kma_orf_index_destroy(kma_orf_index* idx) {
  if (!idx) return KMA_OK;
  DeviceScope ds(idx->device);
  delete idx;
  return KMA_OK;
}

int kma_extend_proposals(const kma_orf_index* idx, const kma_proposal* props, uint64_t n,
                         double min_strength, int min_evidence, int32_t* out_left,
                         int32_t* out_right, uint8_t* out_status, uint64_t* stats) {
  if (!idx || !stats) return fail(KMA_E_INVALID, "null argument");
  stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (n == 0) return KMA_OK;
  if (!props || !out_left || !out_right || !out_status)
    return fail(KMA_E_INVALID, "null argument");
  for (uint64_t i = 0; i < n; ++i) {
    const kma_proposal& p = props[i];
    if (p.contig >= idx->n_contig)
      return fail(KMA_E_INVALID, "proposal %llu: contig %u >= %u", (unsigned long long)i,
                  p.contig, idx->n_contig);
    if (p.strand != '+' && p.strand != '-')
      return fail(KMA_E_INVALID, "proposal %llu: strand must be '+' or '-'",
                  (unsigned long long)i);
    if ((int64_t)p.right - p.left + 1 < 3)
      return fail(KMA_E_INVALID, "proposal %llu: shorter than a codon", (unsigned long long)i);
  }
  DeviceScope ds(idx->device);
  if (int rc = ds.entered()) return rc;
  DevBufs b;
  kma_proposal* d_props;
  kma::OrfExtendArgs a{};
  KMA_HIP(b.alloc(&d_props, n * sizeof(kma_proposal)));
  KMA_HIP(b.alloc(&a.left, n * 4));
  KMA_HIP(b.alloc(&a.right, n * 4));
  KMA_HIP(b.alloc(&a.status, n));
  KMA_HIP(b.alloc(&a.stats, 32));
  a.len = idx->len;
  a.hoff = idx->hoff;
  a.stop_at = idx->stop_at;
  a.start_at = idx->start_at;
  a.props = d_props;
  a.n = n;
  a.min_strength = min_strength;
  a.min_evidence = min_evidence;
  KMA_HIP(hipMemcpy(d_props, props, n * sizeof(kma_proposal), hipMemcpyHostToDevice));
  KMA_HIP(hipMemset(a.stats, 0, 32));
  KMA_HIP(kma::launch_orf_extend(a, nullptr));
  KMA_HIP(hipMemcpy(stats, a.stats, 32, hipMemcpyDeviceToHost));
  KMA_HIP(hipMemcpy(out_left, a.left, n * 4, hipMemcpyDeviceToHost));
  KMA_HIP(hipMemcpy(out_right, a.right, n * 4, hipMemcpyDeviceToHost));
  KMA_HIP(hipMemcpy(out_status, a.status, n, hipMemcpyDeviceToHost));
  return KMA_OK;
}

}  // extern "C"

// ---- protein translation of locations (kma_translate.hip) --------------------------------------
namespace {
thread_local double g_translate_kernel_ms = 0.0;  // the last call's kernel (kma_debug_translate_ms)
}

extern "C" {

int kma_translate_locations(const uint8_t* dna, const uint64_t* offsets, uint32_t n_contig,
                            int genetic_code, int device, const kma_location* locs,
                            uint64_t n_loc, int flags, uint8_t* out_residues, uint64_t cap,
                            uint64_t* out_offsets) {
  g_translate_kernel_ms = 0.0;
  if (!offsets || !out_offsets || (n_loc && !locs)) return fail(KMA_E_INVALID, "null argument");
  if (flags & ~KMA_TR_PEG) return fail(KMA_E_INVALID, "unknown flag bits 0x%x", flags & ~KMA_TR_PEG);
  const char* code = ncbi_code(genetic_code);
  if (!code) return fail(KMA_E_INVALID, "genetic code %d is not a known NCBI table", genetic_code);
  std::vector<uint64_t> off(n_contig + 1ull);
  for (uint32_t c = 0; c < n_contig; ++c) {
    if (offsets[c + 1] < offsets[c]) return fail(KMA_E_INVALID, "offsets decrease at %u", c);
    if (offsets[c + 1] - offsets[0] >= (1ull << 31))
      return fail(KMA_E_INVALID, "2^31 bases or more");
    off[c + 1] = offsets[c + 1] - offsets[0];
  }
  const int64_t drop = flags & KMA_TR_PEG ? 1 : 0;
  out_offsets[0] = 0;
  for (uint64_t i = 0; i < n_loc; ++i) {
    const kma_location& l = locs[i];
    const unsigned long long ii = (unsigned long long)i;
    if (l.contig >= n_contig)
      return fail(KMA_E_INVALID, "location %llu: contig %u >= %u", ii, l.contig, n_contig);
    if (l.strand != '+' && l.strand != '-')
      return fail(KMA_E_INVALID, "location %llu: strand must be '+' or '-'", ii);
    const int64_t n = (int64_t)(off[l.contig + 1] - off[l.contig]);
    if (l.left < 1) return fail(KMA_E_INVALID, "location %llu: left %d < 1", ii, l.left);
    if (l.right > n)
      return fail(KMA_E_INVALID, "location %llu: right %d past the contig's %lld bases", ii,
                  l.right, (long long)n);
    if ((int64_t)l.right < (int64_t)l.left - 1)
      return fail(KMA_E_INVALID, "location %llu: right %d < left %d - 1", ii, l.right, l.left);
    const int64_t codons = ((int64_t)l.right - l.left + 1) / 3 - drop;
    out_offsets[i + 1] = out_offsets[i] + (uint64_t)(codons > 0 ? codons : 0);
  }
  const uint64_t total = out_offsets[n_loc];
  if (total > cap)
    return fail(KMA_E_CAPACITY, "%llu residues, capacity %llu", (unsigned long long)total,
                (unsigned long long)cap);
  if (total == 0) return KMA_OK;
  if (!dna || !out_residues) return fail(KMA_E_INVALID, "null argument");
  DeviceScope ds(device);
  if (int rc = ds.entered()) return rc;
  DevBufs b;
  DevBatch in;  // (off[] is rebased already; a residue to write means there are bases)
  if (int rc = upload_batch(b, dna + offsets[0], off.data(), n_contig, 0, &in)) return rc;
  uint8_t *d_code, *d_out;
  uint64_t* d_ooff;
  kma_location* d_locs;
  KMA_HIP(b.alloc(&d_locs, n_loc * sizeof(kma_location)));
  KMA_HIP(b.alloc(&d_ooff, (n_loc + 1) * 8));
  KMA_HIP(b.alloc(&d_code, 64));
  KMA_HIP(b.alloc(&d_out, total));
  KMA_HIP(hipMemcpy(d_locs, locs, n_loc * sizeof(kma_location), hipMemcpyHostToDevice));
  KMA_HIP(hipMemcpy(d_ooff, out_offsets, (n_loc + 1) * 8, hipMemcpyHostToDevice));
  KMA_HIP(hipMemcpy(d_code, code, 64, hipMemcpyHostToDevice));
  kma::TranslateArgs a{};
  a.dna = in.bytes;
  a.offsets = in.off;
  a.locs = d_locs;
  a.out_off = d_ooff;
  a.n_loc = n_loc;
  a.total = total;
  a.code = d_code;
  a.peg = (uint32_t)(flags & KMA_TR_PEG);
  a.out = d_out;
  struct Events {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Events() {
      for (hipEvent_t x : e)
        if (x) (void)hipEventDestroy(x);
    }
  } ev;
  KMA_HIP(hipEventCreate(&ev.e[0]));
  KMA_HIP(hipEventCreate(&ev.e[1]));
  KMA_HIP(hipEventRecord(ev.e[0], nullptr));
  KMA_HIP(kma::launch_translate(a, nullptr));
  KMA_HIP(hipEventRecord(ev.e[1], nullptr));
  KMA_HIP(hipMemcpy(out_residues, d_out, total, hipMemcpyDeviceToHost));
  float ms = 0.f;
  KMA_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  g_translate_kernel_ms = ms;
  return KMA_OK;
}

// Not in kmeranno.h: measurement hook. hipEvent time of the kernel of this thread's last
// kma_translate_locations call (0 when it launched none).
double kma_debug_translate_ms(void) { return g_translate_kernel_ms; }

}  // extern "C"

// ---- sequence MD5 and the duplicate check (kma_md5.hip) ----------------------------------------
namespace {
constexpr uint64_t kMd5MaxResidues = (1ull << 32) - 128;

// Compute units of `device` (current), asked once per device: the refill form's grid.
int md5_compute_units(int device, uint32_t* n_cu) {
  static std::atomic<uint32_t> known[64];
  if (device >= 0 && device < 64)
    if (const uint32_t c = known[device].load(std::memory_order_relaxed)) return *n_cu = c, KMA_OK;
  int v = 0;
  KMA_HIP(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device));
  *n_cu = (uint32_t)std::max(v, 1);
  if (device >= 0 && device < 64) known[device].store(*n_cu, std::memory_order_relaxed);
  return KMA_OK;
}

// The device entry's checks (no device touched) and its one launch.
int md5_check_device_args(const uint8_t* d_residues, const uint64_t* d_offsets, uint32_t n_seq,
                          uint64_t n_residues, uint32_t flags, const uint8_t* d_digest) {
  if (flags & ~(uint32_t)KMA_MD5_UPPER)
    return fail(KMA_E_INVALID, "unknown flag bits 0x%x", flags & ~(uint32_t)KMA_MD5_UPPER);
  if (n_seq == 0) return KMA_OK;
  if (!d_residues || !d_offsets || !d_digest) return fail(KMA_E_INVALID, "null argument");
  if (n_residues > kMd5MaxResidues)
    return fail(KMA_E_INVALID, "more than 2^32 - 128 residues in one call");
  if (reinterpret_cast<uintptr_t>(d_residues) & 7u)
    return fail(KMA_E_INVALID, "d_residues is not 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_digest) & 15u)
    return fail(KMA_E_INVALID, "d_digest is not 16-byte aligned");
  return KMA_OK;
}

int md5_launch(int device, const uint8_t* d_residues, const uint64_t* d_offsets, uint32_t n_seq,
               uint32_t flags, uint8_t* d_digest, uint32_t form, uint32_t waves_per_cu,
               hipStream_t stream) {
  uint32_t n_cu = 0;
  if (int rc = md5_compute_units(device, &n_cu)) return rc;
  kma::Md5Args a{};
  a.res = d_residues;
  a.off = d_offsets;
  a.n_seq = n_seq;
  a.n_waves = kma::md5_waves(n_seq, form, n_cu, waves_per_cu);
  a.upper = flags & KMA_MD5_UPPER;
  a.digest = reinterpret_cast<uint4*>(d_digest);
  KMA_HIP(kma::launch_md5(a, form, stream));
  return KMA_OK;
}

// The host entries' checks (no device touched).
int md5_check_host_args(const uint8_t* residues, const uint64_t* offsets, uint32_t n_seq,
                        uint32_t flags) {
  if (flags & ~(uint32_t)KMA_MD5_UPPER)
    return fail(KMA_E_INVALID, "unknown flag bits 0x%x", flags & ~(uint32_t)KMA_MD5_UPPER);
  if (n_seq && (!residues || !offsets)) return fail(KMA_E_INVALID, "null argument");
  return check_offsets(offsets, n_seq, "", kMd5MaxResidues + 1,
                       "more than 2^32 - 128 residues in one call");
}
}  // namespace

extern "C" {

int kma_sequence_md5_device(int device, const uint8_t* d_residues, const uint64_t* d_offsets,
                            uint32_t n_seq, uint64_t n_residues, uint32_t flags,
                            uint8_t* d_digest, void* stream) {
  if (int rc = md5_check_device_args(d_residues, d_offsets, n_seq, n_residues, flags, d_digest))
    return rc;
  if (n_seq == 0) return KMA_OK;
  DeviceScope ds(device);
  if (int rc = ds.entered()) return rc;
  return md5_launch(device, d_residues, d_offsets, n_seq, flags, d_digest, kma::kMd5Default, 0,
                    static_cast<hipStream_t>(stream));
}

// Not in kmeranno.h: measurement hook (scripts/md5_rate.py). kma_sequence_md5_device with the
// kernel form (kma_md5.h: kMd5Static | kMd5Coop) and the refill form's waves per compute unit
// (0: the default) chosen by the caller.
int kma_debug_sequence_md5_device(int device, const uint8_t* d_residues,
                                  const uint64_t* d_offsets, uint32_t n_seq, uint64_t n_residues,
                                  uint32_t flags, uint8_t* d_digest, void* stream, uint32_t form,
                                  uint32_t waves_per_cu) {
  if (int rc = md5_check_device_args(d_residues, d_offsets, n_seq, n_residues, flags, d_digest))
    return rc;
  if (form & ~(kma::kMd5Static | kma::kMd5Coop)) return fail(KMA_E_INVALID, "unknown form");
  if (n_seq == 0) return KMA_OK;
  DeviceScope ds(device);
  if (int rc = ds.entered()) return rc;
  return md5_launch(device, d_residues, d_offsets, n_seq, flags, d_digest, form, waves_per_cu,
                    static_cast<hipStream_t>(stream));
}

int kma_sequence_md5(const uint8_t* residues, const uint64_t* offsets, uint32_t n_seq,
                     uint32_t flags, int device, uint8_t* out_digest) {
  if (int rc = md5_check_host_args(residues, offsets, n_seq, flags)) return rc;
  if (n_seq == 0) return KMA_OK;
  if (!out_digest) return fail(KMA_E_INVALID, "null argument");
  DeviceScope ds(device);
  if (int rc = ds.entered()) return rc;
  DevBufs b;
  DevBatch in;
  if (int rc = upload_batch(b, residues, offsets, n_seq, 32, &in)) return rc;
  uint8_t* d_digest;
  KMA_HIP(b.alloc(&d_digest, n_seq * 16ull));
  if (int rc = md5_launch(device, in.bytes, in.off, n_seq, flags, d_digest, kma::kMd5Default, 0,
                          nullptr))
    return rc;
  KMA_HIP(hipMemcpy(out_digest, d_digest, n_seq * 16ull, hipMemcpyDeviceToHost));
  return KMA_OK;
}

int kma_check_sequences(const uint8_t* residues, const uint64_t* offsets, uint32_t n_seq,
                        uint32_t flags, const uint32_t* fun, int device, uint8_t* out_digest,
                        int32_t* out_rep, uint32_t* out_size, uint8_t* out_mixed,
                        uint64_t* out_stats) {
  if (!out_stats) return fail(KMA_E_INVALID, "null argument");
  out_stats[0] = out_stats[1] = out_stats[2] = 0;
  if (int rc = md5_check_host_args(residues, offsets, n_seq, flags)) return rc;
  if (n_seq == 0) return KMA_OK;
  if (!out_rep || !out_size || !out_mixed) return fail(KMA_E_INVALID, "null argument");
  if (n_seq >= (1u << 31)) return fail(KMA_E_INVALID, "2^31 sequences or more");
  DeviceScope ds(device);
  if (int rc = ds.entered()) return rc;
  DevBufs b;
  DevBatch in;
  if (int rc = upload_batch(b, residues, offsets, n_seq, 32, &in)) return rc;
  const uint64_t n = n_seq;
  uint8_t* d_digest;
  uint32_t* d_fun = nullptr;
  kma::SeqCheckArgs a{};
  KMA_HIP(b.alloc(&d_digest, n * 16));
  if (fun) {
    KMA_HIP(b.alloc(&d_fun, n * 4));
    KMA_HIP(hipMemcpy(d_fun, fun, n * 4, hipMemcpyHostToDevice));
  }
  for (uint64_t** p : {&a.key_a, &a.key_b}) KMA_HIP(b.alloc(p, n * 8));
  for (uint32_t** p : {&a.idx_a, &a.idx_b, &a.start, &a.count, &a.fmin, &a.fmax, &a.size})
    KMA_HIP(b.alloc(p, n * 4));
  KMA_HIP(b.alloc(&a.rep, n * 4));
  KMA_HIP(b.alloc(&a.mixed, n));
  KMA_HIP(b.alloc(&a.stats, 24));
  a.digest = reinterpret_cast<const uint4*>(d_digest);
  a.off = in.off;
  a.fun = d_fun;
  a.n = n_seq;
  Scratch tmp;
  KMA_HIP(kma::launch_seq_check(a, nullptr, tmp.ask(), nullptr));
  KMA_HIP(tmp.alloc(b));
  if (int rc = md5_launch(device, in.bytes, in.off, n_seq, flags, d_digest, kma::kMd5Default, 0,
                          nullptr))
    return rc;
  KMA_HIP(kma::launch_seq_check(a, tmp.p, tmp.bytes(), nullptr));
  KMA_HIP(hipMemcpy(out_stats, a.stats, 24, hipMemcpyDeviceToHost));
  KMA_HIP(hipMemcpy(out_rep, a.rep, n * 4, hipMemcpyDeviceToHost));
  KMA_HIP(hipMemcpy(out_size, a.size, n * 4, hipMemcpyDeviceToHost));
  KMA_HIP(hipMemcpy(out_mixed, a.mixed, n, hipMemcpyDeviceToHost));
  if (out_digest) KMA_HIP(hipMemcpy(out_digest, d_digest, n * 16, hipMemcpyDeviceToHost));
  return KMA_OK;
}

}  // extern "C"
