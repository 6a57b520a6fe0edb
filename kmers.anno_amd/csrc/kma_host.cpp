// kma_host.cpp — the host plumbing every unit of the C ABI shares (kma_host.h): the thread's
// error string, the option store and the tuning builds' environment reader, the CPU count and
// the staging pool, small shared helpers, and the operators' batch-setup helpers. The process's
// one instance of each piece of library-wide state lives here.
#include "kma_host.h"

#include <sched.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "kma_internal.h"

namespace kma {
namespace host {

// ---- options (kma_option_set; include/kmeranno.h) ----------------------------------------------
// Library-wide defaults, read per call; workspaces may override the protein-kernel ones. The
// environment is read only by tuning builds (-DKMA_TUNING_ENV=1, the A/B scripts' variants):
// a library a JVM loads must not change its kernel geometry because of a stray variable.
namespace {
constexpr int kNumOpts = 14;  // (number 11 is no option: include/kmeranno.h)
std::atomic<int64_t> g_opt[kNumOpts] = {{0}, {-1}, {0}, {-1}, {0}, {0}, {1}, {0},
                                         {0}, {-1}, {0}, {0}, {0}, {0}};
}  // namespace

bool option_valid(int opt, int64_t v) {
  switch (opt) {
    case KMA_OPT_LAYOUT: return v == -1 || v == 0 || v == 6 || v == 7 || v == (6 | kma::kOrderMod);
    case KMA_OPT_BLOCK_PROTEINS: return v >= 0 && v <= kma::kBlockProteins;
    case KMA_OPT_DEFER: return v >= -1 && v <= 64;
    case KMA_OPT_HOST_PIECES: return v >= 0 && v <= 16;
    case KMA_OPT_HASH_SLICE: return v >= 0;
    case KMA_OPT_PACKED_INPUT: return v >= 0 && v <= 2;
    case KMA_OPT_HOST_THREADS: return v >= 0 && v <= 64;
    case KMA_OPT_HOST_SLICE: return v >= 0 && v <= (int64_t)((1ull << 32) - 128);  // a call's limit
    case KMA_OPT_HOST_PIECE_MIN: return v >= 0 && v <= (int64_t)(1ull << 32);
    case KMA_OPT_PLACEMENT: return v >= -1 && v <= 1;
    case KMA_OPT_HASH_CAP: return v >= 0 && v <= 2048;  // kma_hashindex.h kHashCapMax
    case KMA_OPT_HASH_LDS_KEYS:  // kma_hashsets.h kSetsKeysMin .. kSetsKeysMax
      return v == 0 || (v >= 64 && v <= 4096 && (v & (v - 1)) == 0);
    default: return false;
  }
}

#if KMA_TUNING_ENV
namespace {
struct EnvOptions {  // tuning builds: the A/B scripts' variables seed the defaults once
  EnvOptions() {
    const std::pair<const char*, int> vars[] = {
        {"KMA_MINIMIZER", KMA_OPT_LAYOUT}, {"KMA_BLOCK_PROTEINS", KMA_OPT_BLOCK_PROTEINS},
        {"KMA_DEFER", KMA_OPT_DEFER}, {"KMA_HOST_PIECES", KMA_OPT_HOST_PIECES},
        {"KMA_HASH_SLICE", KMA_OPT_HASH_SLICE}, {"KMA_PACKED_INPUT", KMA_OPT_PACKED_INPUT},
        {"KMA_HOST_THREADS", KMA_OPT_HOST_THREADS}, {"KMA_PLACEMENT", KMA_OPT_PLACEMENT}};
    for (const auto& [name, opt] : vars)
      if (const char* e = getenv(name); e && *e) {
        const int64_t v = strtoll(e, nullptr, 10);
        if (option_valid(opt, v)) g_opt[opt] = v;
      }
  }
} g_env_options;
}  // namespace
#endif

int64_t opt(int o) { return g_opt[o].load(std::memory_order_relaxed); }

// CPUs this process may use: its affinity mask, bounded by a cgroup CPU quota (a container or a
// GPU box granted a share of a machine lists every CPU of the machine in the mask).
static long cgroup_quota_cpus() {
  auto ceil_div = [](long long q, long long p) { return (long)((q + p - 1) / p); };
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // v2: "<quota|max> <period>"
    char q[32] = {};
    long long period = 0;
    const bool ok = fscanf(f, "%31s %lld", q, &period) == 2;
    fclose(f);
    if (ok && strcmp(q, "max") != 0 && period > 0 && atoll(q) > 0) return ceil_div(atoll(q), period);
    return 0;
  }
  long long quota = -1, period = 0;
  if (FILE* f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {  // v1
    if (fscanf(f, "%lld", &quota) != 1) quota = -1;
    fclose(f);
  }
  if (FILE* f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
    if (fscanf(f, "%lld", &period) != 1) period = 0;
    fclose(f);
  }
  return quota > 0 && period > 0 ? ceil_div(quota, period) : 0;
}
size_t host_cores() {
  static const size_t n = [] {
    size_t c = std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof set, &set) == 0 && CPU_COUNT(&set) > 0) c = (size_t)CPU_COUNT(&set);
    const long q = cgroup_quota_cpus();
    return q > 0 ? std::min(c, (size_t)q) : c;
  }();
  return n;
}

// Host threads one staging job (a replica's share of a host call) stages (copies or packs) its
// input with. KMA_OPT_HOST_THREADS is the whole call's budget, split over the replicas the call
// fans out to; by default each of n replicas takes host_cores() / n, at most 16 (packing 5 bits
// per residue keeps up with one PCIe link on ~16 threads). Round 5 gave every replica min(16,
// cores): an 8-replica call ran 8 jobs of 16 on one pool of at most 63 threads.
size_t staging_width(int n_replicas) {
  const size_t n = (size_t)std::max(1, n_replicas);
  const int64_t o = opt(KMA_OPT_HOST_THREADS);
  if (o > 0) return std::max<size_t>(1, (size_t)o / n);
  return std::clamp<size_t>(host_cores() / n, 1, 16);
}
// The width of the staging jobs of the calling thread: set for a replica's shard thread by the
// host call that fans out (ShardWidth), else a one-replica call's.
thread_local size_t t_shard_width = 0;
size_t staging_threads() { return t_shard_width ? t_shard_width : staging_width(1); }

StagingPool& staging_pool() {
  static StagingPool* pool = new StagingPool();  // never destroyed: no join at process exit
  return *pool;
}

// dst[i] = src[i] - base for i < n, on the staging pool for large n (a host call's rebased
// offsets: 8 MB for c5's 1M proteins).
void rebase_offsets(uint64_t* dst, const uint64_t* src, uint64_t n, uint64_t base) {
  constexpr uint64_t kChunk = 1u << 17;
  staging_pool().run((n + kChunk - 1) / kChunk, n >= 4 * kChunk ? staging_threads() : 1,
                     [&](uint64_t c) {
                       const uint64_t e = std::min(n, (c + 1) * kChunk);
                       for (uint64_t i = c * kChunk; i < e; ++i) dst[i] = src[i] - base;
                     });
}

// The first s < n with offsets[s + 1] < offsets[s], or n: chunks on the staging pool, each a
// branch-free (vectorized) pass (c5's 1M offsets: a serial scan with an early exit per element
// ran ~0.5 ms before the call's first copy).
uint32_t offsets_decrease_at(const uint64_t* offsets, uint32_t n) {
  constexpr uint64_t kChunk = 1u << 16;
  const uint64_t n_chunks = (n + kChunk - 1) / kChunk;
  std::vector<uint8_t> bad(n_chunks);
  staging_pool().run(n_chunks, n >= 4 * kChunk ? staging_threads() : 1, [&](uint64_t c) {
    const uint64_t e = std::min<uint64_t>(n, (c + 1) * kChunk);
    uint64_t b = 0;
    for (uint64_t i = c * kChunk; i < e; ++i) b |= offsets[i + 1] < offsets[i];
    bad[c] = b != 0;
  });
  for (uint64_t c = 0; c < n_chunks; ++c)
    if (bad[c])
      for (uint64_t i = c * kChunk; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return (uint32_t)i;
  return n;
}

// memcpy on the staging pool in 1 MiB chunks (the outputs of a large host call).
void pool_memcpy(void* dst, const void* src, size_t n) {
  constexpr size_t kChunk = 1u << 20;
  staging_pool().run((n + kChunk - 1) / kChunk, n >= 4 * kChunk ? staging_threads() : 1,
                     [&](uint64_t c) {
                       const size_t o = c * kChunk;
                       std::memcpy(static_cast<uint8_t*>(dst) + o,
                                   static_cast<const uint8_t*>(src) + o, std::min(kChunk, n - o));
                     });
}

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

void standard_lut(uint8_t lut[256]) {
  std::memset(lut, 0, 256);
  for (int c = 'A'; c <= 'Z'; ++c) lut[c] = (uint8_t)(c - 'A' + 1);
  lut[(uint8_t)'*'] = 27;
}

int check_k(int k) {
  if (k < 1 || k > KMA_MAX_K) return fail(KMA_E_INVALID, "kmer size %d outside 1..%d", k, KMA_MAX_K);
  return KMA_OK;
}

// NCBI translation tables, codons in T, C, A, G order.
const char* ncbi_code(int gc) {
  switch (gc) {
    case 1: case 11: return "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
    case 2: return "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSS**VVVVAAAADDEEGGGG";
    case 3: return "FFLLSSSSYY**CCWWTTTTPPPPHHQQRRRRIIMMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
    case 4: return "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
    case 5: return "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSSSSVVVVAAAADDEEGGGG";
    case 6: return "FFLLSSSSYYQQCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
    case 9: return "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNNKSSSSVVVVAAAADDEEGGGG";
    case 10: return "FFLLSSSSYY**CCCWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
    case 12: return "FFLLSSSSYY**CC*WLLLSPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
    case 13: return "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSSGGVVVVAAAADDEEGGGG";
    case 14: return "FFLLSSSSYYY*CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNNKSSSSVVVVAAAADDEEGGGG";
    case 16: return "FFLLSSSSYY*LCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
    case 21: return "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNNKSSSSVVVVAAAADDEEGGGG";
    case 22: return "FFLLSS*SYY*LCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
    case 23: return "FF*LSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
    case 24: return "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSSKVVVVAAAADDEEGGGG";
    case 25: return "FFLLSSSSYY**CCGWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
    default: return nullptr;
  }
}

// Contiguous shards [b[i], b[i+1]) of n units (proteins, contigs) with near-equal payload
// (residues, bases): cut where the payload prefix crosses i/parts of the total.
std::vector<uint32_t> shard_bounds(const uint64_t* off, uint32_t n, int parts) {
  std::vector<uint32_t> b(parts + 1, 0);
  b[parts] = n;
  const uint64_t base = off[0], total = off[n] - base;
  for (int i = 1; i < parts; ++i) {
    const uint64_t target = base + (uint64_t)((double)total * i / parts);
    const uint64_t* it = std::lower_bound(off + 1, off + n + 1, target);
    b[i] = std::max(b[i - 1], std::min(n, (uint32_t)(it - off)));
  }
  return b;
}

// ---- batch setup of the one-shot operators (kma_host.h) -----------------------------------------
int check_offsets(const uint64_t* offsets, uint32_t n, const char* what, uint64_t limit,
                  const char* too_long) {
  for (uint32_t s = 0; s < n; ++s)
    if (offsets[s + 1] < offsets[s])
      return fail(KMA_E_INVALID, "%s%soffsets decrease at %u", what, *what ? " " : "", s);
  if (n && limit && offsets[n] - offsets[0] >= limit) return fail(KMA_E_INVALID, "%s", too_long);
  return KMA_OK;
}

int upload_batch(DevBufs& b, const uint8_t* bytes, const uint64_t* offsets, uint32_t n,
                 uint64_t pad, DevBatch* out) {
  const uint64_t base = offsets[0];
  std::vector<uint64_t> rel(offsets, offsets + n + 1);
  for (auto& o : rel) o -= base;
  out->total = rel[n];
  KMA_HIP(b.alloc(&out->bytes, out->total + pad));
  KMA_HIP(b.alloc(&out->off, (n + 1) * 8ull));
  if (out->total) KMA_HIP(hipMemcpy(out->bytes, bytes + base, out->total, hipMemcpyHostToDevice));
  if (pad) KMA_HIP(hipMemset(out->bytes + out->total, 0, pad));
  KMA_HIP(hipMemcpy(out->off, rel.data(), (n + 1) * 8ull, hipMemcpyHostToDevice));
  return KMA_OK;
}

}  // namespace host
}  // namespace kma

using namespace kma::host;

extern "C" {

int kma_abi_version(void) { return KMA_ABI_VERSION; }

int kma_option_set(int option, int64_t value) {
  if (option < 1 || option >= kNumOpts || !option_valid(option, value))
    return fail(KMA_E_INVALID, "option %d: value %lld out of range", option, (long long)value);
  g_opt[option] = value;
  return KMA_OK;
}

int kma_option_get(int option, int64_t* value) {
  if (!value || option < 1 || option >= kNumOpts || option == 11)
    return fail(KMA_E_INVALID, "option %d unknown (or null value)", option);
  *value = opt(option);
  return KMA_OK;
}

const char* kma_last_error(void) { return g_err.c_str(); }

int kma_device_count(int* out_n) {
  if (!out_n) return fail(KMA_E_INVALID, "null out_n");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *out_n = 0;
    return fail(KMA_E_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *out_n = n;
  return KMA_OK;
}

// Not in kmeranno.h: the CPUs the library sizes its staging jobs by (host_cores).
int kma_debug_host_cores(void) { return (int)host_cores(); }

}  // extern "C"
