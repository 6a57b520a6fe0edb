// kma_abi_table.cpp — the table half of the C ABI (include/kmeranno.h): the creators and their
// layout rule, both device builds, replication, wrap / build-device, info, destroy, and the
// per-table pool of host contexts (kma_objects.h) the host entry points draw from.
//
// Host-side orchestration only: argument checks, key packing, device allocation and copies,
// replica management and kernel launches (kma_build.hip). No compute falls back to the CPU:
// without a usable HIP device every entry point that needs one returns KMA_E_DEVICE.
#include <chrono>

#include "kma_internal.h"
#include "kma_objects.h"
#include "kma_tsv.h"

using namespace kma::host;

namespace {
// The forced table layout (KMA_OPT_LAYOUT): -1 = not forced.
int forced_layout() { return (int)opt(KMA_OPT_LAYOUT); }
// Table creators try two-choice placement first for narrow tables (KMA_OPT_PLACEMENT -1 / 1);
// 0 builds chains only.
bool two_choice_first(int k) { return !kma::wide_k(k) && opt(KMA_OPT_PLACEMENT) != 0; }
}  // namespace

// The size rule's minimizer code (m | order): m = min(K, 6) up to kMinimizer6Buckets buckets,
// else min(K, 7); K = 8, m = 6 tables take the mod-sampling order (kma_internal.h kOrderMod:
// fewer home-line requests per window). Until the order's single-residue form and the cheaper
// bucket match it was kept to tables beyond the Infinity Cache (its VALU slowed the 6-frame
// probe on the cache-resident 10^7 table); since then the 10^7 table measures c4 2.284 vs
// 2.763 ms, c2 42.4-42.8 vs 43.4-43.6 us, c3's probe 72.7-72.8 vs 72.9-73.2 us in it
// (profiles/r06/order_small_tables_r06j/). KMA_OPT_LAYOUT forces a code (6: the random order).
int kma::minimizer_len(int k, uint64_t n_buckets) {
  const int m6 = k < 6 ? k : 6, m7 = k < 7 ? k : 7;
  const int f = forced_layout();
  if (f == 0) return 0;
  if (f == 6) return m6;
  if (f == 7) return m7;
  if (f == (6 | kma::kOrderMod)) return kma::order_mod_valid(k, 6) ? 6 | kma::kOrderMod : m6;
  const uint64_t lim = kma::wide_k(k) ? kma::kMinimizer6BucketsWide : kma::kMinimizer6Buckets;
  const int m = n_buckets <= lim ? m6 : m7;
  return kma::order_mod_valid(k, m) ? m | kma::kOrderMod : m;
}

namespace {
using kma::kMaxBuckets;

// Slot array geometry of a table of K-mers: narrow (K <= 8, kSlotsPerBucket u64 slots per
// bucket) or wide (K 9..12, four 16-byte slots per 64-byte bucket; kma_internal.h).
uint64_t bucket_bytes(int k) { return kma::wide_k(k) ? 64u : (uint64_t)kma::kBucketBytes; }
uint64_t buckets_for_k(uint64_t n_keys, double load_factor, int k) {
  if (load_factor <= 0) load_factor = 0.5;
  const int spb = kma::slots_for_k(k);
  const double slots = (double)(n_keys ? n_keys : 1) / load_factor;
  const uint64_t nb = (uint64_t)((slots + spb - 1) / spb);
  return nb < 1 ? 1 : nb;
}

// Pack rows [lo, hi) with the LUT; 0 for rows of the wrong length or with unencodable bytes.
void pack_rows(const uint8_t* lut, const char* text, const uint64_t* off, uint64_t lo, uint64_t hi,
               int k, uint64_t* keys) {
  for (uint64_t r = lo; r < hi; ++r) {
    const uint64_t b = off[r], e = off[r + 1];
    uint64_t key = 0;
    if (e - b == (uint64_t)k) {
      for (int j = 0; j < k; ++j) {
        const uint8_t c = lut[(uint8_t)text[b + j]];
        if (!c) {
          key = 0;
          break;
        }
        key = (key << 5) | c;
      }
    }
    keys[r] = key;
  }
}

template <class F>
void parallel_rows(uint64_t n, F f) {
  unsigned nt = (unsigned)std::min<size_t>(16, host_cores());
  if (n < (1u << 16)) nt = 1;
  std::vector<std::thread> th;
  const uint64_t chunk = (n + nt - 1) / nt;
  for (unsigned t = 0; t < nt; ++t) {
    const uint64_t lo = t * chunk, hi = std::min(n, lo + chunk);
    if (lo < hi) th.emplace_back(f, lo, hi);
  }
  for (auto& x : th) x.join();
}

void destroy_ctx(HostCtx* c) {
  DeviceScope ds(c->device);
  if (c->ws) kma_workspace_destroy(c->ws);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  for (hipStream_t cs : c->copy)
    if (cs) (void)hipStreamDestroy(cs);
  if (c->d2h) (void)hipStreamDestroy(c->d2h);
  for (hipEvent_t* ev : {c->piece_ready, c->piece_ready2, c->piece_done, c->out_ready})
    for (int i = 0; i < kMaxPieces; ++i)
      if (ev[i]) (void)hipEventDestroy(ev[i]);
  c->d_in.release();
  c->d_off.release();
  c->d_out.release();
  c->d_aux.release();
  c->d_hits.release();
  c->h_in.release();
  c->h_out.release();
  delete c;
}
}  // namespace

// Take a host context for `device` from the table's pool (or make one).
int kma::host::acquire_ctx(kma_table* t, int device, HostCtx** out) {
  {
    std::lock_guard<std::mutex> g(t->pool_mu);
    for (size_t i = 0; i < t->idle.size(); ++i)
      if (t->idle[i]->device == device) {
        *out = t->idle[i];
        t->idle.erase(t->idle.begin() + i);
        return KMA_OK;
      }
  }
  DeviceScope ds(device);
  if (ds.err != hipSuccess) return fail(KMA_E_DEVICE, "hipSetDevice(%d)", device);
  HostCtx* c = new HostCtx();
  c->device = device;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  for (hipStream_t& cs : c->copy)
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->d2h, hipStreamNonBlocking);
  for (hipEvent_t* ev : {c->piece_ready, c->piece_ready2, c->piece_done, c->out_ready})
    for (int i = 0; i < kMaxPieces && e == hipSuccess; ++i)
      e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
  if (e != hipSuccess) {
    destroy_ctx(c);
    return fail(KMA_E_DEVICE, "stream / event create: %s", hipGetErrorString(e));
  }
  if (int rc = kma_workspace_create(device, &c->ws)) {
    destroy_ctx(c);
    return rc;
  }
  c->ws->host_ctx = true;
  *out = c;
  return KMA_OK;
}
void kma::host::release_ctx(kma_table* t, HostCtx* c) {
  std::lock_guard<std::mutex> g(t->pool_mu);
  t->idle.push_back(c);
}

// A copy of the table's replicas (safe against a concurrent kma_table_replicate).
std::vector<Replica> kma::host::replicas(const kma_table* t) {
  std::lock_guard<std::mutex> g(t->reps_mu);
  return t->reps;
}
bool kma::host::replica_on(const kma_table* t, int device, Replica* out) {
  std::lock_guard<std::mutex> g(t->reps_mu);
  for (const Replica& r : t->reps)
    if (r.device == device) {
      *out = r;
      return true;
    }
  return false;
}

namespace {
int add_replica(kma_table* t, int device, uint64_t* d_slots, bool owned) {
  Replica r;
  r.device = device;
  r.d_slots = d_slots;
  r.owned = owned;
  DeviceScope ds(device);
  if (ds.err != hipSuccess) return fail(KMA_E_DEVICE, "hipSetDevice(%d)", device);
  hipError_t e = hipMalloc(&r.d_lut, 256);
  if (e == hipSuccess) e = hipMemcpy(r.d_lut, t->lut, 256, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (r.d_lut) (void)hipFree(r.d_lut);
    return fail(KMA_E_DEVICE, "table LUT upload: %s", hipGetErrorString(e));
  }
  std::lock_guard<std::mutex> g(t->reps_mu);
  t->reps.push_back(r);
  t->info.n_replicas = (int32_t)t->reps.size();
  return KMA_OK;
}

kma_table* new_table(int device, int k, int m, uint64_t n_buckets, const uint8_t lut[256],
                     bool two_choice = false) {
  kma_table* t = new kma_table();
  t->k = k;
  t->mlen = m;
  t->two_choice = two_choice;
  t->info.two_choice = two_choice ? 1 : 0;
  t->n_buckets = n_buckets;
  std::memcpy(t->lut, lut, 256);
  t->info.n_buckets = n_buckets;
  t->info.bytes = n_buckets * bucket_bytes(k);
  t->info.slots_per_bucket = kma::slots_for_k(k);
  t->info.k = k;
  t->info.device = device;
  t->info.minimizer_len = m & kma::kMinimizerMask;
  t->info.minimizer_order = (m & kma::kOrderMod) ? 1 : 0;
  int ne = 0;
  for (int c = 0; c < 256; ++c)
    if (lut[c] >= 28) t->info.extra_syms[lut[c] - 28] = (uint8_t)c, ++ne;
  t->info.n_extra_syms = ne;
  return t;
}

void free_table(kma_table* t) {
  for (HostCtx* c : t->idle) destroy_ctx(c);
  for (Replica& r : t->reps) {
    DeviceScope ds(r.device);
    if (r.owned && r.d_slots) (void)hipFree(r.d_slots);
    if (r.d_lut) (void)hipFree(r.d_lut);
  }
  delete t;
}

int build_on_device(uint64_t* d_slots, uint64_t n_buckets, int k, int m, uint32_t* d_winner,
                    const uint64_t* d_keys, const uint32_t* d_fids, uint64_t n, uint32_t* d_status,
                    hipStream_t s) {
  if (n_buckets >= kMaxBuckets) return fail(KMA_E_INVALID, "%llu buckets or more",
                                           (unsigned long long)kMaxBuckets);
  KMA_HIP(hipMemsetAsync(d_slots, 0, n_buckets * bucket_bytes(k), s));
  KMA_HIP(hipMemsetAsync(d_winner, 0, n_buckets * kma::slots_for_k(k) * sizeof(uint32_t), s));
  KMA_HIP(hipMemsetAsync(d_status, 0, 4 * sizeof(uint32_t), s));
  KMA_HIP(kma::launch_build_insert(d_slots, d_winner, (uint32_t)n_buckets, k, m, d_keys, n,
                                   d_status, s));
  KMA_HIP(kma::launch_build_finalize(d_slots, d_winner, d_fids, (uint32_t)n_buckets, k, m,
                                     d_status + 1, s));
  return KMA_OK;
}

// Two-choice build (kma_build.hip launch_build_two_choice) into zeroed slots on stream s; its
// sort buffers are allocated here and freed after the stream has drained them.
int build_two_choice_on_device(uint64_t* d_slots, uint64_t n_buckets, int k, int m,
                               const uint64_t* d_keys, const uint32_t* d_fids, uint64_t n,
                               uint32_t* d_status, hipStream_t s) {
  if (n_buckets >= kMaxBuckets) return fail(KMA_E_INVALID, "%llu buckets or more",
                                           (unsigned long long)kMaxBuckets);
  if (n_buckets < 2) return fail(KMA_E_INVALID, "two-choice placement needs 2 buckets or more");
  if (n >= (1ull << 32)) return fail(KMA_E_INVALID, "2^32 rows or more");
  KMA_HIP(hipMemsetAsync(d_slots, 0, n_buckets * bucket_bytes(k), s));
  KMA_HIP(hipMemsetAsync(d_status, 0, 4 * sizeof(uint32_t), s));
  if (n == 0) return KMA_OK;
  size_t temp_bytes = 0;
  kma::TwoChoiceScratch x;
  KMA_HIP(kma::launch_build_two_choice(d_slots, (uint32_t)n_buckets, k, m, d_keys, d_fids, n,
                                       nullptr, nullptr, nullptr, x, nullptr, &temp_bytes,
                                       d_status, s));
  DevBufs tmp;
  uint64_t* skeys;
  uint32_t *rows, *srows;
  void* temp;
  KMA_HIP(tmp.alloc(&skeys, n * 8));
  KMA_HIP(tmp.alloc(&rows, n * 4));
  KMA_HIP(tmp.alloc(&srows, n * 4));
  KMA_HIP(tmp.alloc(&temp, temp_bytes));
  KMA_HIP(tmp.alloc(&x.home, n * 4));  // home-first placement (kma_build.hip)
  KMA_HIP(tmp.alloc(&x.sorted_home, n * 4));
  KMA_HIP(tmp.alloc(&x.sorted_idx, n * 4));
  KMA_HIP(tmp.alloc(&x.away, n));
#ifndef KMA_TC_ALT_LOAD
#define KMA_TC_ALT_LOAD 1
#endif
  if (KMA_TC_ALT_LOAD) KMA_HIP(tmp.alloc(&x.load, n_buckets));
  KMA_HIP(kma::launch_build_two_choice(d_slots, (uint32_t)n_buckets, k, m, d_keys, d_fids, n,
                                       skeys, rows, srows, x, temp, &temp_bytes, d_status, s));
  KMA_HIP(hipStreamSynchronize(s));  // before DevBufs frees the sort buffers
  return KMA_OK;
}
}  // namespace

// Table from device-resident keys/fids on `device` (n rows; fids already checked). Narrow tables
// are built with two-choice placement first (round 5; KMA_OPT_PLACEMENT 0 skips it), at the size
// rule's layout (a crowded minimizer table also flat, kept if it halves the displaced keys).
// Chained tables (wide K, or a two-choice build that failed) are laid out by the size rule and
// then by measurement (kma_internal.h, kRetryDisplaced / kMaxDisplaced): an m = 6 table with
// many displaced keys is rebuilt with m = 7 (kept if it displaces fewer), a still crowded
// minimizer table is rebuilt flat (kept if that halves the displaced keys or the longest
// chain). KMA_OPT_LAYOUT forces a layout.
int kma::host::create_from_device_keys(const uint64_t* d_keys, const uint32_t* d_fids, uint64_t n,
                                       int k, int device, double lf, const uint8_t lut[256],
                                       kma_table** out) {
  const uint64_t nb = buckets_for_k(n, lf, k);
  if (nb >= kMaxBuckets)
    return fail(KMA_E_INVALID, "table too large: %llu buckets", (unsigned long long)nb);
  DevBufs tmp;
  uint32_t *d_winner, *d_status;
  KMA_HIP(tmp.alloc(&d_winner, nb * kma::slots_for_k(k) * 4));
  KMA_HIP(tmp.alloc(&d_status, 16));
  auto build = [&](int m, uint64_t** slots, uint32_t st[4]) -> int {
    KMA_HIP(hipMalloc(slots, nb * bucket_bytes(k)));
    int rc = build_on_device(*slots, nb, k, m, d_winner, d_keys, d_fids, n, d_status, nullptr);
    if (rc == KMA_OK) {
      hipError_t e = hipMemcpy(st, d_status, 16, hipMemcpyDeviceToHost);
      if (e != hipSuccess) rc = fail(KMA_E_DEVICE, "build: %s", hipGetErrorString(e));
      else if (st[0]) rc = fail(KMA_E_TABLE_FULL, "signature table full");
    }
    if (rc != KMA_OK) {
      (void)hipFree(*slots);
      *slots = nullptr;
    }
    return rc;
  };
  int m = kma::minimizer_len(k, nb);
  uint64_t* d_slots = nullptr;
  uint32_t st[4] = {};
  auto displaced = [](const uint32_t s[4]) { return (double)s[3] / std::max<uint32_t>(s[1], 1); };
  if (two_choice_first(k) && nb >= 2) {
    // Two-choice placement at the size rule's (or the forced) layout; a crowded minimizer table
    // is also built flat and the flat one kept if it halves the displaced keys; a minimizer build
    // that fails (an insertion exceeded kMaxKicks) is retried flat; a build that still fails
    // falls through to the chained rule below.
    uint32_t s2[4] = {};
    auto build2 = [&](int m2, uint64_t** slots, uint32_t out[4]) -> int {
      KMA_HIP(hipMalloc(slots, nb * bucket_bytes(k)));
      int rc = build_two_choice_on_device(*slots, nb, k, m2, d_keys, d_fids, n, d_status, nullptr);
      if (rc == KMA_OK) {
        hipError_t e = hipMemcpy(out, d_status, 16, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(KMA_E_DEVICE, "build: %s", hipGetErrorString(e));
      }
      if (rc != KMA_OK || out[0]) {
        (void)hipFree(*slots);
        *slots = nullptr;
      }
      return rc;
    };
    uint64_t* d2 = nullptr;
    if (int rc = build2(m, &d2, s2)) return rc;
    if (s2[0] && m != 0 && forced_layout() < 0) {
      // A minimizer table whose insertions ran out of evictions (keys piling onto few
      // minimizers: their homes full, so they all compete for alternates) is built flat with
      // two-choice placement before falling back to chains: adversarial keys sharing 2,000
      // minimizers at LF 0.9 got a flat chained table with chains of 30 buckets
      // (profiles/r05/robustness_r05k.jsonl).
      if (int rc = build2(0, &d2, s2)) return rc;
      if (!s2[0]) m = 0;  // (else the chained rule below starts from the size rule's m)
    }
    if (!s2[0]) {  // built
      d_slots = d2;
      std::memcpy(st, s2, sizeof st);
      if (forced_layout() < 0 && m != 0 && displaced(st) > kma::kMaxDisplacedTwoChoice) {
        uint64_t* d3 = nullptr;
        uint32_t s3[4] = {};
        if (int rc = build2(0, &d3, s3)) {
          (void)hipFree(d_slots);
          return rc;
        }
        if (d3 && 2ull * s3[3] < st[3]) {
          (void)hipFree(d_slots);
          d_slots = d3;
          std::memcpy(st, s3, sizeof st);
          m = 0;
        } else if (d3) {
          (void)hipFree(d3);
        }
      }
      kma_table* t = new_table(device, k, m, nb, lut, true);
      if (int rc = add_replica(t, device, d_slots, true)) {
        (void)hipFree(d_slots);
        delete t;
        return rc;
      }
      t->info.n_rows = n;
      t->info.n_entries = st[1];
      t->info.max_probe = st[2];
      t->info.n_displaced = st[3];
      *out = t;
      return KMA_OK;
    }
  }
  if (int rc = build(m, &d_slots, st)) return rc;
  // Replace the current table (slots, stats, m) by a build with layout m2 when keep() says so.
  auto try_layout = [&](int m2, bool (*keep)(const uint32_t*, const uint32_t*)) -> int {
    uint64_t* d2 = nullptr;
    uint32_t s2[4] = {};
    if (int rc = build(m2, &d2, s2)) {
      (void)hipFree(d_slots);
      return rc;
    }
    const bool better = keep(st, s2);
    (void)hipFree(better ? d_slots : d2);
    if (better) {
      d_slots = d2;
      std::memcpy(st, s2, sizeof st);
      m = m2;
    }
    return KMA_OK;
  };
  const int m6 = std::min(k, 6), m7 = std::min(k, 7);
  if (forced_layout() < 0) {
    if ((m & kma::kMinimizerMask) == m6 && m6 != m7 && displaced(st) > kma::kRetryDisplaced)
      if (int rc = try_layout(m7, [](const uint32_t* a, const uint32_t* b) { return b[3] < a[3]; }))
        return rc;
    const bool crowded = displaced(st) > kma::kMaxDisplaced || st[2] > kma::kMaxChain;
    if (m != 0 && crowded)
      if (int rc = try_layout(0, [](const uint32_t* a, const uint32_t* b) {
            return 2ull * b[3] < a[3] || (a[2] > kma::kMaxChain && 2 * b[2] < a[2]);
          }))
        return rc;
  }
  kma_table* t = new_table(device, k, m, nb, lut);
  if (int rc = add_replica(t, device, d_slots, true)) {
    (void)hipFree(d_slots);
    delete t;
    return rc;
  }
  t->info.n_rows = n;
  t->info.n_entries = st[1];
  t->info.max_probe = st[2];
  t->info.n_displaced = st[3];
  *out = t;
  return KMA_OK;
}

namespace {
// Shared by both create forms: keys packed on the host with `lut`.
int create_from_keys(const std::vector<uint64_t>& keys, const uint32_t* fids, uint64_t n, int k,
                     int device, double lf, const uint8_t lut[256], uint64_t n_skipped,
                     kma_table** out) {
  if (lf <= 0) lf = 0.5;
  if (lf > 0.95) return fail(KMA_E_INVALID, "load factor %.3f > 0.95", lf);
  for (uint64_t r = 0; r < n; ++r)
    if (fids[r] > KMA_MAX_FID) return fail(KMA_E_INVALID, "fid %u of row %llu exceeds 2^22-1",
                                            fids[r], (unsigned long long)r);
  DeviceScope ds(device);
  if (int rc = ds.entered()) return rc;
  DevBufs tmp;
  uint64_t* d_keys;
  uint32_t* d_fids;
  KMA_HIP(tmp.alloc(&d_keys, n * 8));
  KMA_HIP(tmp.alloc(&d_fids, n * 4));
  KMA_HIP(hipMemcpy(d_keys, keys.data(), n * 8, hipMemcpyHostToDevice));
  KMA_HIP(hipMemcpy(d_fids, fids, n * 4, hipMemcpyHostToDevice));
  const int rc = create_from_device_keys(d_keys, d_fids, n, k, device, lf, lut, out);
  if (rc != KMA_OK) return rc;
  (*out)->info.n_skipped = n_skipped;
  return KMA_OK;
}

// A layout code (kma_table_build_device / kma_table_wrap_device) -> minimizer code (m | order)
// and placement. -1 is kma_table_layout_for's code for (k, n_buckets) in both entry points, so a
// table built with -1 and wrapped with -1 agree (a caller whose -1 build reports a failed
// two-choice insertion rebuilds with an explicit chained code and wraps with that code).
int resolve_layout(int k, uint64_t n_buckets, int layout, int* m, bool* two) {
  const int code = layout < 0 ? kma::minimizer_len(k, n_buckets) |
                                    (two_choice_first(k) && n_buckets >= 2 ? kma::kLayoutTwoChoice : 0)
                              : layout;
  if (code & ~(kma::kLayoutMask | kma::kLayoutTwoChoice))
    return fail(KMA_E_INVALID, "layout code %d has unknown bits", layout);
  *m = code & kma::kLayoutMask;
  *two = (code & kma::kLayoutTwoChoice) != 0;
  const int mm = *m & kma::kMinimizerMask;
  if ((*m & ~kma::kMinimizerMask) & ~kma::kOrderMod)
    return fail(KMA_E_INVALID, "layout code %d has unknown bits", layout);
  if ((*m & kma::kOrderMod) ? !kma::order_mod_valid(k, *m)
                            : (mm != 0 && mm != std::min(k, 6) && mm != std::min(k, 7)))
    return fail(KMA_E_INVALID,
                "layout %d is not 0, min(K, 6) or min(K, 7) (| mod-sampling: K = 8, m = 6)", layout);
  if (*two && kma::wide_k(k)) return fail(KMA_E_INVALID, "two-choice placement takes K <= 8");
  return KMA_OK;
}

}  // namespace

extern "C" {

uint64_t kma_table_buckets_for(uint64_t n_keys, double load_factor) {
  return buckets_for_k(n_keys, load_factor, kma::kMaxNarrowK);
}

uint64_t kma_table_buckets_for_k(uint64_t n_keys, double load_factor, int k) {
  return buckets_for_k(n_keys, load_factor, k);
}

int kma_bucket_slots_for(int k) { return check_k(k) ? 0 : kma::slots_for_k(k); }

int kma_table_layout_for(int k, uint64_t n_buckets) {
  return kma::minimizer_len(k, n_buckets) |
         (two_choice_first(k) && n_buckets >= 2 ? kma::kLayoutTwoChoice : 0);
}

int kma_bucket_slots(void) { return kma::kSlotsPerBucket; }

int kma_pack_kmers(const kma_table* table, const char* text, const uint64_t* offsets, uint64_t n,
                   uint64_t* out_keys) {
  if (!table || (!text && n) || !offsets || (!out_keys && n))
    return fail(KMA_E_INVALID, "null argument");
  pack_rows(table->lut, text, offsets, 0, n, table->k, out_keys);
  return KMA_OK;
}

int kma_table_create(const char* text, const uint64_t* offsets, const uint32_t* fids, uint64_t n,
                     int k, int device, double load_factor, kma_table** out) {
  if (!out || (n && (!text || !offsets || !fids))) return fail(KMA_E_INVALID, "null argument");
  if (int rc = check_k(k)) return rc;
  // Alphabet: standard A-Z and '*', plus up to four other bytes found in K-length rows.
  bool seen[256] = {};
  for (uint64_t r = 0; r < n; ++r)
    if (offsets[r + 1] - offsets[r] == (uint64_t)k)
      for (uint64_t i = offsets[r]; i < offsets[r + 1]; ++i) seen[(uint8_t)text[i]] = true;
  uint8_t lut[256];
  standard_lut(lut);
  int extra = 0;
  for (int c = 0; c < 256; ++c)
    if (seen[c] && !lut[c]) {
      if (extra == 4) return fail(KMA_E_ALPHABET, "more than 4 kmer symbols outside [A-Z*]");
      lut[c] = (uint8_t)(28 + extra++);
    }
  std::vector<uint64_t> keys(n);
  parallel_rows(n, [&](uint64_t lo, uint64_t hi) {
    pack_rows(lut, text, offsets, lo, hi, k, keys.data());
  });
  uint64_t skipped = 0;
  for (uint64_t r = 0; r < n; ++r) skipped += offsets[r + 1] - offsets[r] != (uint64_t)k;
  return create_from_keys(keys, fids, n, k, device, load_factor, lut, skipped, out);
}

int kma_table_create_from_tsv(const char* path, int k, int n_devices, const int* device_ids,
                              double load_factor, kma_table** out, char** role_names,
                              uint64_t* role_bytes, uint32_t* n_roles, int* last_kmer_len) {
  if (!path || !out || n_devices < 1 || !device_ids) return fail(KMA_E_INVALID, "null argument");
  *out = nullptr;
  if (role_names) *role_names = nullptr;
  if (int rc = check_k(k)) return rc;
  // the alphabet rule of kma_table_create: A-Z and '*', then up to four other bytes of K-length
  // kmers in byte order
  auto make_lut = [](const bool* seen, uint8_t* lut) {
    standard_lut(lut);
    int extra = 0;
    for (int c = 0; c < 256; ++c)
      if (seen[c] && !lut[c]) {
        if (extra == 4) return KMA_E_ALPHABET;
        lut[c] = (uint8_t)(28 + extra++);
      }
    return KMA_OK;
  };
  kma::KmerTsv tsv;
  std::string err;
  if (int rc = kma::read_kmer_tsv(path, k, (unsigned)std::min<size_t>(16, host_cores()), make_lut,
                                  &tsv, &err))
    return fail(rc, "%s", err.c_str());
  kma_table* t = nullptr;
  if (int rc = create_from_keys(tsv.keys, tsv.fids.data(), tsv.keys.size(), k, device_ids[0],
                                load_factor, tsv.lut, tsv.n_skipped, &t))
    return rc;
  if (n_devices > 1)
    if (int rc = kma_table_replicate(t, n_devices - 1, device_ids + 1)) {
      free_table(t);
      return rc;
    }
  uint64_t bytes = 0;
  for (const std::string& r : tsv.roles) bytes += r.size() + 1;
  if (role_names) {
    char* blob = static_cast<char*>(malloc(std::max<uint64_t>(bytes, 1)));
    if (!blob) {
      free_table(t);
      return fail(KMA_E_NOMEM, "role names: %llu bytes", (unsigned long long)bytes);
    }
    char* p = blob;
    for (const std::string& r : tsv.roles) {
      std::memcpy(p, r.data(), r.size());
      p += r.size();
      *p++ = '\0';
    }
    *role_names = blob;
  }
  if (role_bytes) *role_bytes = bytes;
  if (n_roles) *n_roles = (uint32_t)tsv.roles.size();
  if (last_kmer_len) *last_kmer_len = tsv.last_kmer_len;
  *out = t;
  return KMA_OK;
}

void kma_free(void* p) { free(p); }

int kma_table_create_packed(const uint64_t* keys, const uint32_t* fids, uint64_t n, int k,
                            int device, double load_factor, kma_table** out) {
  if (!out || (n && (!keys || !fids))) return fail(KMA_E_INVALID, "null argument");
  if (int rc = check_k(k)) return rc;
  uint8_t lut[256];
  standard_lut(lut);
  std::vector<uint64_t> kv(keys, keys + n);
  uint64_t skipped = 0;
  const uint64_t lim = 1ull << (5 * k);
  for (uint64_t r = 0; r < n; ++r)
    if (kv[r] == 0 || kv[r] >= lim) kv[r] = 0, ++skipped;
  return create_from_keys(kv, fids, n, k, device, load_factor, lut, skipped, out);
}

int kma_table_replicate(kma_table* t, int n_devices, const int* device_ids) {
  if (!t || n_devices < 0 || (n_devices && !device_ids) || replicas(t).empty())
    return fail(KMA_E_INVALID, "null argument");
  const Replica src = replicas(t)[0];
  const uint64_t bytes = t->n_buckets * bucket_bytes(t->k);
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess) return fail(KMA_E_DEVICE, "hipGetDeviceCount");
  for (int i = 0; i < n_devices; ++i)
    if (device_ids[i] < 0 || device_ids[i] >= n_dev)
      return fail(KMA_E_INVALID, "device %d not present", device_ids[i]);
  // Every destination's slot array and copy stream first; then all copies at once (each on its
  // destination's stream, so each GPU's copy engine pulls replica 0 over its own xGMI link
  // instead of one link at a time); then one wait for all of them.
  struct Dest {
    int dev;
    uint64_t* d = nullptr;
    hipStream_t s = nullptr;
    bool peer = false;  // the destination reads replica 0 directly (peer access enabled)
  };
  std::vector<Dest> dst(n_devices);
  auto cleanup = [&](bool free_slots) {
    for (Dest& x : dst) {
      DeviceScope ds(x.dev);
      if (x.s) (void)hipStreamDestroy(x.s);
      if (free_slots && x.d) (void)hipFree(x.d);
      x.s = nullptr;
    }
  };
  for (int i = 0; i < n_devices; ++i) {
    Dest& x = dst[i];
    x.dev = device_ids[i];
    DeviceScope ds(x.dev);
    hipError_t e = ds.err;
    if (e == hipSuccess) e = hipMalloc(&x.d, bytes);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&x.s, hipStreamNonBlocking);
    if (e == hipSuccess && x.dev != src.device) {
      // Peer access from the destination to replica 0's device, once per pair (an enabled pair
      // stays enabled): its copy engine then pulls the slot array over xGMI. Without it the
      // runtime may stage a peer copy through host memory.
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, x.dev, src.device) == hipSuccess && can) {
        const hipError_t pe = hipDeviceEnablePeerAccess(src.device, 0);
        if (pe == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
        x.peer = pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled;
      }
    }
    if (e != hipSuccess) {
      cleanup(true);
      return fail(e == hipErrorOutOfMemory ? KMA_E_NOMEM : KMA_E_DEVICE,
                  "replica on device %d: %s", x.dev, hipGetErrorString(e));
    }
  }
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t e = hipSuccess;
  for (Dest& x : dst) {
    DeviceScope ds(x.dev);
    e = x.dev == src.device
            ? hipMemcpyAsync(x.d, src.d_slots, bytes, hipMemcpyDeviceToDevice, x.s)
            : hipMemcpyPeerAsync(x.d, x.dev, src.d_slots, src.device, bytes, x.s);
    if (e != hipSuccess) break;
  }
  for (Dest& x : dst) {
    DeviceScope ds(x.dev);
    const hipError_t w = hipStreamSynchronize(x.s);  // every issued copy, even after a failure
    if (e == hipSuccess) e = w;
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (e != hipSuccess) {
    cleanup(true);
    return fail(KMA_E_DEVICE, "replica copies: %s", hipGetErrorString(e));
  }
  cleanup(false);
  for (size_t i = 0; i < dst.size(); ++i)
    if (int rc = add_replica(t, dst[i].dev, dst[i].d, true)) {
      for (size_t j = i; j < dst.size(); ++j) {
        DeviceScope ds(dst[j].dev);
        (void)hipFree(dst[j].d);
      }
      return rc;
    }
  std::lock_guard<std::mutex> g(t->reps_mu);
  t->info.replicate_ms = ms;
  t->info.replicate_bytes = bytes * (uint64_t)n_devices;
  t->info.replicate_peer = 0;
  t->info.replicate_local = 0;
  for (const Dest& x : dst) {
    t->info.replicate_peer += x.peer ? 1 : 0;
    t->info.replicate_local += x.dev == src.device ? 1 : 0;
  }
  return KMA_OK;
}

int kma_table_create_replicated(const char* text, const uint64_t* offsets, const uint32_t* fids,
                                uint64_t n, int k, int n_devices, const int* device_ids,
                                double load_factor, kma_table** out) {
  if (!out || n_devices < 1 || !device_ids) return fail(KMA_E_INVALID, "null argument");
  *out = nullptr;
  kma_table* t = nullptr;
  if (int rc = kma_table_create(text, offsets, fids, n, k, device_ids[0], load_factor, &t))
    return rc;
  if (int rc = kma_table_replicate(t, n_devices - 1, device_ids + 1)) {
    free_table(t);
    return rc;
  }
  *out = t;
  return KMA_OK;
}

int kma_table_replicas(const kma_table* t, int* n, int* device_ids, int cap) {
  if (!t || !n) return fail(KMA_E_INVALID, "null argument");
  const std::vector<Replica> reps = replicas(t);
  *n = (int)reps.size();
  for (int i = 0; i < *n && i < cap && device_ids; ++i) device_ids[i] = reps[i].device;
  return KMA_OK;
}

int kma_table_info_get(const kma_table* table, kma_table_info* out) {
  if (!table || !out) return fail(KMA_E_INVALID, "null argument");
  std::lock_guard<std::mutex> g(table->reps_mu);  // kma_table_replicate writes n_replicas
  *out = table->info;
  return KMA_OK;
}

int kma_table_destroy(kma_table* table) {
  if (!table) return KMA_OK;
  free_table(table);
  return KMA_OK;
}

int kma_table_build_device(void* d_slots, uint64_t n_buckets, int k, int layout,
                           uint32_t* d_winner, const uint64_t* d_keys, const uint32_t* d_fids,
                           uint64_t n, uint32_t* d_status, void* stream) {
  if (int rc = check_k(k)) return rc;
  if (!n_buckets) return fail(KMA_E_INVALID, "null argument");
  int m = 0;
  bool two = false;
  if (int rc = resolve_layout(k, n_buckets, layout, &m, &two)) return rc;
  // d_winner is the chained build's scratch; a two-choice build does not read it.
  if (!d_slots || (!two && !d_winner) || !d_status || (n && (!d_keys || !d_fids)))
    return fail(KMA_E_INVALID, "null argument");
  if (two) {
    return build_two_choice_on_device(static_cast<uint64_t*>(d_slots), n_buckets, k, m, d_keys,
                                      d_fids, n, d_status, static_cast<hipStream_t>(stream));
  }
  return build_on_device(static_cast<uint64_t*>(d_slots), n_buckets, k, m, d_winner, d_keys,
                         d_fids, n, d_status, static_cast<hipStream_t>(stream));
}

int kma_table_wrap_device(void* d_slots, uint64_t n_buckets, int k, int layout, int device,
                          kma_table** out) {
  if (!d_slots || !out || !n_buckets) return fail(KMA_E_INVALID, "null argument");
  if (n_buckets >= kMaxBuckets) return fail(KMA_E_INVALID, "%llu buckets or more",
                                           (unsigned long long)kMaxBuckets);
  if (int rc = check_k(k)) return rc;
  int m = 0;
  bool two = false;
  if (int rc = resolve_layout(k, n_buckets, layout, &m, &two)) return rc;
  if (two && n_buckets < 2)
    return fail(KMA_E_INVALID, "two-choice placement takes K <= 8 and 2 buckets or more");
  uint8_t lut[256];
  standard_lut(lut);
  kma_table* t = new_table(device, k, m, n_buckets, lut, two);
  if (int rc = add_replica(t, device, static_cast<uint64_t*>(d_slots), false)) {
    delete t;
    return rc;
  }
  *out = t;
  return KMA_OK;
}

int kma_table_device_ptr(const kma_table* table, void** d_slots, uint64_t* bytes) {
  if (!table || !d_slots || !bytes || replicas(table).empty())
    return fail(KMA_E_INVALID, "null argument");
  *d_slots = replicas(table)[0].d_slots;
  *bytes = table->n_buckets * bucket_bytes(table->k);
  return KMA_OK;
}

}  // extern "C"
