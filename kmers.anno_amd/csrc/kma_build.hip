// kma_build.hip — table construction and the sort-and-scan builders for CDNA4 (gfx950). The
// rocPRIM calls (radix sort, select, scan) live here, away from the probe units.
//
//   build_insert / build_finalize  signature-table construction (ApplyKmerProcessor.java:100-110)
//   build_two_choice_*             two-choice placement of a narrow table
//   peg_windows / singleton_flags / build_windows / signature_flags  table builders (A9, (f)1)
#include <cstring>  // (rocprim.hpp uses memset without including it)
#include <rocprim/rocprim.hpp>

#include <algorithm>

#include "../../include/kmeranno.h"
#include "kma_internal.h"
#include "kma_device.h"

namespace kma {
namespace {

// ---------------------------------------------------------------------------------------------
// Table construction. Insert: claim the first empty slot of the probe chain with a 64-bit CAS
// (slot key bits, fid still 0; the slot's overflow bit may already be set) or find the key
// already there; either way record the row index with atomicMax so the LAST row of a duplicate
// key wins (HashMap.put semantics). A key placed past its home bucket sets its overflow bit
// there. Finalize: write the winning row's fid into the slot; collect entry count, longest
// chain and the number of keys displaced past their home bucket.
// ---------------------------------------------------------------------------------------------
// Wide tables (K > 8): the same with 16-byte slots (kma_internal.h): the claim is a 64-bit CAS
// of the slot's key words (x | y << 32, 0 = empty), the overflow bit and fid live in .z.
template <bool Wide>
__global__ __launch_bounds__(256) void build_insert_kernel(uint64_t* slots, uint32_t* winner,
                                                           uint32_t n_buckets, int k, int m,
                                                           const uint64_t* __restrict__ keys,
                                                           uint64_t n, uint32_t* status) {
  constexpr int S = Wide ? kWideSlots : kSlotsPerBucket;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t key = keys[i];
    if (key == 0 || (key >> (5 * k)) != 0) continue;  // no key / not a K-mer key: never stored
    const uint64_t want = Wide ? key : slot_make(key, 0);
    const uint32_t home = home_bucket(key, k, m, n_buckets);
    uint32_t b = home;
    bool done = false;
    for (uint32_t p = 0; p < n_buckets && !done; ++p) {
      b = chain_bucket(home, p, n_buckets);
      for (int j = 0; j < S; ++j) {
        const uint64_t si = (uint64_t)b * S + j;
        uint64_t* sp = slots + (Wide ? 2 * si : si);
        uint64_t v = __hip_atomic_load(sp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (Wide) {
          while (v == 0) {  // empty: claim it
            const uint64_t old = atomicCAS((unsigned long long*)sp, 0ull, (unsigned long long)want);
            v = old == 0 ? want : old;
          }
        } else {
          while ((uint32_t)v == 0u) {  // empty (possibly with its overflow bit set): claim it
            const uint64_t old = atomicCAS((unsigned long long*)sp, (unsigned long long)v, v | want);
            v = old == v ? (v | want) : old;
          }
        }
        if ((Wide ? v : slot_key(v)) == key) {
          atomicMax(winner + si, (uint32_t)(i + 1));
          done = true;
          break;
        }
      }
    }
    if (!done) {
      atomicOr(status, 1u);  // table full: cannot happen at load factor < 1
    } else if (b != home) {  // displaced: set the key's filter positions in its home bucket
      for (int f = 0; f < kFilterBits; ++f) {
        const uint32_t pos = filter_pos<S>((uint32_t)key, f);
        const uint64_t si = (uint64_t)home * S + pos / kFilterBits;
        uint32_t* meta = Wide ? reinterpret_cast<uint32_t*>(slots + 2 * si + 1)   // .z
                              : reinterpret_cast<uint32_t*>(slots + si) + 1;      // high dword
        const uint32_t bit = 1u << (kFidBits + pos % kFilterBits);
        if (!(__hip_atomic_load(meta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit))
          atomicOr(meta, bit);
      }
    }
  }
}

template <bool Wide>
__global__ __launch_bounds__(256) void build_finalize_kernel(uint64_t* slots,
                                                             const uint32_t* __restrict__ winner,
                                                             const uint32_t* __restrict__ fids,
                                                             uint32_t n_buckets, int k, int m,
                                                             uint32_t* stats) {
  constexpr int S = Wide ? kWideSlots : kSlotsPerBucket;
  const uint64_t n_slots = (uint64_t)n_buckets * S;
  uint32_t entries = 0, max_probe = 0, displaced = 0;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_slots;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t w = winner[i];
    if (w == 0) continue;
    uint64_t key;
    if (Wide) {
      key = slots[2 * i];
      uint32_t* meta = reinterpret_cast<uint32_t*>(slots + 2 * i + 1);
      *meta = *meta | (fids[w - 1] & kFidMask);  // keep the filter bits
    } else {
      const uint64_t v = slots[i];
      slots[i] = v | ((uint64_t)(fids[w - 1] & kFidMask) << 32);
      key = slot_key(v);
    }
    const uint32_t b = (uint32_t)(i / S), h = home_bucket(key, k, m, n_buckets);
    const uint32_t d = chain_step(h, b, n_buckets) + 1u;
    entries++;
    displaced += d > 1u ? 1u : 0u;
    max_probe = max(max_probe, d);
  }
  entries = wave_sum(entries);
  max_probe = wave_max(max_probe);
  displaced = wave_sum(displaced);
  if ((threadIdx.x & 63) == 0) {
    if (entries) atomicAdd(stats + 0, entries);
    atomicMax(stats + 1, max_probe);
    if (displaced) atomicAdd(stats + 2, displaced);
  }
}

// ---------------------------------------------------------------------------------------------
// Two-choice build (narrow tables; kma_internal.h alt_bucket). The rows are radix-sorted by key
// with their row index (stable: a key's rows stay in file order), so the last row of every run
// is the row HashMap.put keeps; each such key is inserted into an empty slot of its home or alt
// bucket, or evicts a pseudo-random slot of a full one and carries the victim to the victim's
// other bucket (a random-walk cuckoo insertion; every slot exchange is one 64-bit atomic, so no
// key is lost or doubled). A key still in hand after kMaxKicks evictions marks the build failed
// (the caller builds the table with chains instead). The filter pass then sets, for every key
// stored in its alt bucket, its filter positions in its home bucket, and counts.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void iota_kernel(uint32_t* rows, uint64_t n) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x)
    rows[i] = (uint32_t)i;
}

__device__ __forceinline__ bool claim_empty(uint64_t* slots, uint32_t b, uint64_t v) {
  uint64_t* sp = slots + (uint64_t)b * kSlotsPerBucket;
#pragma unroll
  for (int j = 0; j < kSlotsPerBucket; ++j)
    if (__hip_atomic_load(sp + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull &&
        atomicCAS((unsigned long long*)(sp + j), 0ull, (unsigned long long)v) == 0ull)
      return true;
  return false;
}

__global__ __launch_bounds__(256) void build_two_choice_insert_kernel(
    uint64_t* slots, uint32_t n_buckets, int k, int m, const uint64_t* __restrict__ skeys,
    const uint32_t* __restrict__ srows, const uint32_t* __restrict__ fids, uint64_t n,
    const uint8_t* __restrict__ away, uint8_t phase, uint32_t* status) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    if (away && away[i] != phase) continue;  // phase 0: the keys kept home; 1: the others
    const uint64_t key = skeys[i];
    if (key == 0 || (key >> (5 * k)) != 0) continue;  // no key / not a K-mer key: never stored
    if (i + 1 < n && skeys[i + 1] == key) continue;   // a later row of this key wins
    uint64_t v = slot_make(key, fids[srows[i]]);
    uint32_t b1 = home_bucket(key, k, m, n_buckets);
    uint32_t b2 = alt_bucket(key, b1, n_buckets);
    uint32_t at = b1;  // the bucket to evict from when both are full
    uint32_t rng = (uint32_t)i * 0x9E3779B1u + 0x7F4A7C15u;
    bool done = false;
    for (uint32_t kick = 0; kick <= kMaxKicks; ++kick) {
      if (claim_empty(slots, b1, v) || claim_empty(slots, b2, v)) {
        done = true;
        break;
      }
      if (kick == kMaxKicks) break;
      rng = rng * 1664525u + 1013904223u;
      const uint32_t j = rng >> (32 - kSlotBits);
      const uint64_t old = atomicExch((unsigned long long*)(slots + (uint64_t)at * kSlotsPerBucket + j),
                                      (unsigned long long)v);
      if (old == 0ull) {  // (slots never empty again once claimed; kept for safety)
        done = true;
        break;
      }
      // the victim lived in `at`: its other bucket first (then `at`, for a slot freed meanwhile)
      v = old;
      const uint64_t vk = slot_key(old);
      const uint32_t h = home_bucket(vk, k, m, n_buckets);
      const uint32_t other = at == h ? alt_bucket(vk, h, n_buckets) : h;
      b1 = other;
      b2 = at;
      at = other;
    }
    if (!done) atomicOr(status, 1u);
  }
}

// Home-first placement: the keys of a home bucket that cannot all live there are
// chosen before any insertion. home_kernel: the home of every key the insert kernel stores (the
// last row of its run, a K-mer key), else kNoHome, with its sorted-key index; the pairs are then
// radix-sorted by home, and select_kernel takes each home's run: up to kSlotsPerBucket keys stay
// (away = 0: inserted first, into the home, where they all fit), the others go away (away = 1:
// inserted after every home is filled, so into their alt buckets, evicting only where an alt
// is full). The keys sent away are chosen greedily to set few filter positions in the home: each
// next one adds the fewest positions not yet set (first 64 keys of a run; the rest go away as
// they come). Against insertion order: c5 (10^8 keys, m = 6) simulated 2.8% -> 1.35% false
// filter hits per missed window; measured displaced keys 7.50 -> 7.18% (a key sent to a full
// alt still evicts), c5 kernel 3.124 -> 3.085 ms, LF 0.75 3.42 -> 3.37 ms (ABAB,
// profiles/r05/tc_select_ab/; without the scratch buffers insertion order decides). Keys whose alt is
// already filled by that bucket's own home keys go away last (each would evict one of them, a
// second displaced key): displaced 7.18 -> 6.99% at LF 0.5 and 17.55 -> 15.49% at 0.75, c5
// kernel 3.095 -> 3.084 and 3.374 -> 3.283 ms (profiles/r05/tc_alt_load_ab/; KMA_TC_ALT_LOAD=0).
constexpr uint32_t kNoHome = 0xFFFFFFFFu;
__global__ __launch_bounds__(256) void build_two_choice_home_kernel(
    const uint64_t* __restrict__ skeys, uint64_t n, int k, int m, uint32_t n_buckets,
    uint32_t* __restrict__ home, uint32_t* __restrict__ idx) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t key = skeys[i];
    const bool stored = key != 0 && (key >> (5 * k)) == 0 && !(i + 1 < n && skeys[i + 1] == key);
    home[i] = stored ? home_bucket(key, k, m, n_buckets) : kNoHome;
    idx[i] = (uint32_t)i;
  }
}
// Keys homed per bucket (capped at 255), from the runs of the sorted homes (zeroed before).
__global__ __launch_bounds__(256) void build_two_choice_load_kernel(
    const uint32_t* __restrict__ hs, uint64_t n, uint8_t* __restrict__ load) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t h = hs[i];
    if (h == kNoHome || (i > 0 && hs[i - 1] == h)) continue;
    uint64_t e = i + 1;
    while (e < n && hs[e] == h && e - i < 255) ++e;
    load[h] = (uint8_t)(e - i);
  }
}
__global__ __launch_bounds__(256) void build_two_choice_select_kernel(
    const uint32_t* __restrict__ hs, const uint32_t* __restrict__ ids,
    const uint64_t* __restrict__ skeys, uint64_t n, const uint8_t* __restrict__ load,
    uint32_t n_buckets, uint8_t* __restrict__ away) {
  constexpr uint32_t S = kSlotsPerBucket;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t h = hs[i];
    if (h == kNoHome) {
      away[ids[i]] = 2;  // not stored: neither phase
      continue;
    }
    // Past a run's first 64 keys (the run is contiguous: hs[i - 64] == h) a key goes away as it
    // comes, written by its own thread; a run's first thread decides its first W <= 64 keys. (One
    // thread per run walking the whole run was O(run) work: keys piling onto one home made the
    // build a single-thread job)
    if (i >= 64 && hs[i - 64] == h) {
      away[ids[i]] = 1;
      continue;
    }
    if (i > 0 && hs[i - 1] == h) continue;  // within the first 64: the run's first thread
    uint64_t e = i + 1;
    while (e < n && hs[e] == h && e - i < 64) ++e;
    const uint32_t W = (uint32_t)(e - i);
    for (uint64_t j = i; j < e; ++j) away[ids[j]] = 0;
    if (W <= S) continue;
    uint64_t chosen = 0;
    uint32_t set = 0;
    for (uint32_t it = 0; it < W - S; ++it) {
      uint32_t best = 0, best_new = 64, best_mask = 0;
      for (uint32_t j = 0; j < W; ++j) {
        if (chosen >> j & 1ull) continue;
        const uint64_t key = skeys[ids[i + j]];
        const uint32_t mask = filter_need<S>((uint32_t)key);
        // a key whose alt is filled by its own home keys would evict one of them (a second key
        // displaced): such keys go last
        const bool alt_full = load && load[alt_bucket(key, h, n_buckets)] >= S;
        const uint32_t fresh = (uint32_t)__popc(mask & ~set) + (alt_full ? 32u : 0u);
        if (fresh < best_new) {
          best = j;
          best_new = fresh;
          best_mask = mask;
          if (fresh == 0) break;
        }
      }
      chosen |= 1ull << best;
      set |= best_mask;
      away[ids[i + best]] = 1;
    }
  }
}

__global__ __launch_bounds__(256) void build_two_choice_filter_kernel(uint64_t* slots,
                                                                      uint32_t n_buckets, int k,
                                                                      int m, uint32_t* stats) {
  constexpr int S = kSlotsPerBucket;
  const uint64_t n_slots = (uint64_t)n_buckets * S;
  uint32_t entries = 0, displaced = 0;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_slots;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t v = __hip_atomic_load(slots + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((uint32_t)v == 0u) continue;
    const uint64_t key = slot_key(v);
    const uint32_t b = (uint32_t)(i / S), h = home_bucket(key, k, m, n_buckets);
    entries++;
    if (b != h) {  // in its alt bucket: its filter positions in the home bucket
      displaced++;
      for (int f = 0; f < kFilterBits; ++f) {
        const uint32_t pos = filter_pos<S>((uint32_t)key, f);
        uint32_t* meta = reinterpret_cast<uint32_t*>(slots + (uint64_t)h * S + pos / kFilterBits) + 1;
        const uint32_t bit = 1u << (kFidBits + pos % kFilterBits);
        // read first: keys displaced from one crowded home would otherwise serialize on the
        // same words (one atomic each)
        if (!(__hip_atomic_load(meta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit))
          atomicOr(meta, bit);
      }
    }
  }
  entries = wave_sum(entries);
  displaced = wave_sum(displaced);
  if ((threadIdx.x & 63) == 0) {
    if (entries) atomicAdd(stats + 0, entries);
    atomicMax(stats + 1, displaced ? 2u : entries ? 1u : 0u);
    if (displaced) atomicAdd(stats + 2, displaced);
  }
}

// Peg windows (KmerReference.countPegKmers, KmerReference.java:124-147): one wave per peg;
// position i of peg s gets the packed key of window [i, i + K) if i < L - K (end exclusive)
// and the window has no 'X' and only standard symbols (others can never equal a translated
// contig kmer), else 0; every position of the batch is written.
__global__ __launch_bounds__(256) void peg_windows_kernel(const uint8_t* __restrict__ residues,
                                                          const uint64_t* __restrict__ offsets,
                                                          uint32_t n_peg, int k,
                                                          const uint8_t* __restrict__ lut_g,
                                                          uint64_t* __restrict__ keys,
                                                          uint32_t* __restrict__ pegs) {
  __shared__ uint8_t lut[256];
  lut[threadIdx.x] = threadIdx.x == 'X' ? 0 : lut_g[threadIdx.x];  // 'X' windows are skipped
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t o0 = offsets[0];
  for (uint64_t s = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < n_peg;
       s += (uint64_t)gridDim.x * 4) {
    const uint64_t lo = offsets[s], hi = offsets[s + 1];
    const int64_t end = (int64_t)(hi - lo) - k;  // windows i < end
    for (uint64_t p = lo + lane; p < hi; p += 64) {
      const int64_t i = (int64_t)(p - lo);
      uint64_t key = 0;
      if (i < end) {
        bool ok = true;
        for (int j = 0; j < k; ++j) {
          const uint32_t c = lut[residues[p + j]];
          ok = ok && c != 0u;
          key = (key << 5) | c;
        }
        key = ok ? key : 0;
      }
      keys[p - o0] = key;
      pegs[p - o0] = (uint32_t)s;
    }
  }
}

__global__ __launch_bounds__(256) void singleton_flags_kernel(const uint64_t* __restrict__ k,
                                                              uint64_t n,
                                                              uint8_t* __restrict__ flags) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * 256) {
    const uint64_t v = k[i];
    flags[i] = v != 0 && (i == 0 || k[i - 1] != v) && (i + 1 == n || k[i + 1] != v);
  }
}

// Signature build (BuildKmerProcessor.java:137-223). One wave per protein: every window of
// ProteinKmers (i = 0..L-K, or i < L-K with end_exclusive) of an interesting peg (role >= 0) or
// a buffered protein (role -1) becomes (key, role or kBuildNeg); every other position gets key 0.
// A window with a byte the standard alphabet cannot encode raises alpha_flag (the host refuses
// the batch rather than drop a kmer the reference would keep). Keys are up to 60 bits (K <= 12).
__global__ __launch_bounds__(256) void build_windows_kernel(const uint8_t* __restrict__ residues,
                                                            const uint64_t* __restrict__ offsets,
                                                            uint32_t n_seq,
                                                            const int32_t* __restrict__ roles,
                                                            int k, int end_exclusive,
                                                            const uint8_t* __restrict__ lut_g,
                                                            uint64_t* __restrict__ keys,
                                                            uint32_t* __restrict__ tags,
                                                            uint32_t* __restrict__ alpha_flag) {
  __shared__ uint8_t lut[256];
  lut[threadIdx.x] = lut_g[threadIdx.x];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t o0 = offsets[0];
  for (uint64_t s = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < n_seq;
       s += (uint64_t)gridDim.x * 4) {
    const uint64_t lo = offsets[s], hi = offsets[s + 1];
    const int32_t role = roles[s];
    const int64_t n_win = (int64_t)(hi - lo) - k + (end_exclusive ? 0 : 1);
    const bool counted = role >= -1;
    const uint32_t tag = role >= 0 ? (uint32_t)role : kBuildNeg;
    bool bad = false;
    for (uint64_t p = lo + lane; p < hi; p += 64) {
      const int64_t i = (int64_t)(p - lo);
      uint64_t v = 0;
      if (counted && i < n_win) {
        uint64_t key = 0;
        bool ok = true;
        for (int j = 0; j < k; ++j) {
          const uint32_t c = lut[residues[p + j]];
          ok = ok && c != 0u;
          key = (key << 5) | c;
        }
        bad = bad || !ok;
        v = ok ? key : 0;
      }
      keys[p - o0] = v;
      tags[p - o0] = tag;
    }
    if (__ballot(bad) && lane == 0) atomicOr(alpha_flag, 1u);
  }
}

// RoleCounter over the (key, role) pairs sorted by key (RoleCounter.java:42-56: a kmer is good
// iff every count hit its first role; BuildKmerProcessor.java:191-208 removes kmers of buffered
// proteins). Pass 1: a run's first pair is flagged, and its index is the run id of every pair
// of the run (max-scan of head indices). Pass 2: a pair whose role differs from its run's
// first, or that comes from a buffered protein, clears the run's flag.
__global__ __launch_bounds__(256) void sig_heads_kernel(const uint64_t* __restrict__ k, uint64_t n,
                                                        uint8_t* __restrict__ flags,
                                                        uint32_t* __restrict__ head_idx) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * 256) {
    const uint64_t v = k[i];
    const bool head = v != 0 && (i == 0 || k[i - 1] != v);
    flags[i] = head ? 1 : 0;
    head_idx[i] = head ? (uint32_t)i : 0u;
  }
}

__global__ __launch_bounds__(256) void sig_clear_kernel(const uint64_t* __restrict__ k,
                                                        const uint32_t* __restrict__ tags,
                                                        const uint32_t* __restrict__ run,
                                                        uint64_t n, uint8_t* __restrict__ flags) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * 256) {
    if (k[i] == 0) continue;
    const uint32_t h = run[i], t = tags[i];
    if (t == kBuildNeg || t != tags[h]) flags[h] = 0;  // every writer stores 0
  }
}

}  // namespace

// ---- launchers ----------------------------------------------------------------------------------
static unsigned grid_for(uint64_t n, unsigned cap = 8192) {
  uint64_t g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

hipError_t launch_build_insert(uint64_t* slots, uint32_t* winner, uint32_t n_buckets, int k,
                               int m, const uint64_t* keys, uint64_t n, uint32_t* status,
                               hipStream_t stream) {
  if (wide_k(k))
    hipLaunchKernelGGL(build_insert_kernel<true>, dim3(grid_for(n)), dim3(256), 0, stream, slots,
                       winner, n_buckets, k, m, keys, n, status);
  else
    hipLaunchKernelGGL(build_insert_kernel<false>, dim3(grid_for(n)), dim3(256), 0, stream, slots,
                       winner, n_buckets, k, m, keys, n, status);
  return hipGetLastError();
}

hipError_t launch_build_finalize(uint64_t* slots, const uint32_t* winner, const uint32_t* fids,
                                 uint32_t n_buckets, int k, int m, uint32_t* stats,
                                 hipStream_t stream) {
  const dim3 g(grid_for((uint64_t)n_buckets * slots_for_k(k)));
  if (wide_k(k))
    hipLaunchKernelGGL(build_finalize_kernel<true>, g, dim3(256), 0, stream, slots, winner, fids,
                       n_buckets, k, m, stats);
  else
    hipLaunchKernelGGL(build_finalize_kernel<false>, g, dim3(256), 0, stream, slots, winner, fids,
                       n_buckets, k, m, stats);
  return hipGetLastError();
}

hipError_t launch_build_two_choice(uint64_t* slots, uint32_t n_buckets, int k, int m,
                                   const uint64_t* keys, const uint32_t* fids, uint64_t n,
                                   uint64_t* sorted_keys, uint32_t* rows, uint32_t* sorted_rows,
                                   const TwoChoiceScratch& x, void* temp, size_t* temp_bytes,
                                   uint32_t* status, hipStream_t stream) {
  if (wide_k(k) || n_buckets < 2) return hipErrorInvalidValue;
  // all 64 bits: a row whose key is not a K-mer key (bits above 5K) must not split a run
  if (!temp) {
    size_t t1 = 0, t2 = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, t1, keys, sorted_keys, rows, sorted_rows,
                                             (size_t)n, 0u, 64u, stream);
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(nullptr, t2, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                  (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0u, 32u,
                                  stream);
    *temp_bytes = std::max(t1, t2);
    return e;
  }
  hipLaunchKernelGGL(iota_kernel, dim3(grid_for(n)), dim3(256), 0, stream, rows, n);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = rocprim::radix_sort_pairs(temp, *temp_bytes, keys, sorted_keys, rows, sorted_rows, (size_t)n,
                                0u, 64u, stream);
  if (e != hipSuccess) return e;
  if (x.home) {
    hipLaunchKernelGGL(build_two_choice_home_kernel, dim3(grid_for(n)), dim3(256), 0, stream,
                       sorted_keys, n, k, m, n_buckets, x.home, rows);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(temp, *temp_bytes, x.home, x.sorted_home, rows, x.sorted_idx,
                                  (size_t)n, 0u, 32u, stream);
    if (e != hipSuccess) return e;
    if (x.load) {
      if ((e = hipMemsetAsync(x.load, 0, n_buckets, stream)) != hipSuccess) return e;
      hipLaunchKernelGGL(build_two_choice_load_kernel, dim3(grid_for(n)), dim3(256), 0, stream,
                         x.sorted_home, n, x.load);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(build_two_choice_select_kernel, dim3(grid_for(n)), dim3(256), 0, stream,
                       x.sorted_home, x.sorted_idx, sorted_keys, n, x.load, n_buckets, x.away);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const uint8_t* away = x.away;
  for (uint8_t phase = 0; phase < (away ? 2 : 1); ++phase) {
    hipLaunchKernelGGL(build_two_choice_insert_kernel, dim3(grid_for(n)), dim3(256), 0, stream,
                       slots, n_buckets, k, m, sorted_keys, sorted_rows, fids, n, away, phase,
                       status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(build_two_choice_filter_kernel, dim3(grid_for((uint64_t)n_buckets * kSlotsPerBucket)),
                     dim3(256), 0, stream, slots, n_buckets, k, m, status + 1);
  return hipGetLastError();
}

hipError_t launch_peg_windows(const uint8_t* residues, const uint64_t* offsets, uint32_t n_peg,
                              int k, const uint8_t* lut, uint64_t* keys, uint32_t* pegs,
                              hipStream_t stream) {
  const unsigned g = (unsigned)std::min<uint64_t>(8192, ((uint64_t)n_peg + 3) / 4);
  hipLaunchKernelGGL(peg_windows_kernel, dim3(g ? g : 1), dim3(256), 0, stream, residues,
                     offsets, n_peg, k, lut, keys, pegs);
  return hipGetLastError();
}

hipError_t launch_sort_pairs(void* temp, size_t* temp_bytes, const uint64_t* keys_in,
                             uint64_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out,
                             uint64_t n, int key_bits, hipStream_t stream) {
  return rocprim::radix_sort_pairs(temp, *temp_bytes, keys_in, keys_out, vals_in, vals_out,
                                   (size_t)n, 0u, (unsigned)key_bits, stream);
}

hipError_t launch_singleton_flags(const uint64_t* sorted_keys, uint64_t n, uint8_t* flags,
                                  hipStream_t stream) {
  hipLaunchKernelGGL(singleton_flags_kernel, dim3(grid_for(n)), dim3(256), 0, stream,
                     sorted_keys, n, flags);
  return hipGetLastError();
}

hipError_t launch_select_flagged(void* temp, size_t* temp_bytes, const uint64_t* keys_in,
                                 const uint32_t* vals_in, const uint8_t* flags, uint64_t* keys_out,
                                 uint32_t* vals_out, uint64_t* n_out, uint64_t n,
                                 hipStream_t stream) {
  // Keys and values: two passes over the same flags keep the order identical.
  size_t need = 0;
  hipError_t e = rocprim::select(nullptr, need, keys_in, flags, keys_out, n_out, (size_t)n,
                                 stream);
  if (e != hipSuccess) return e;
  size_t need2 = 0;
  e = rocprim::select(nullptr, need2, vals_in, flags, vals_out, n_out, (size_t)n, stream);
  if (e != hipSuccess) return e;
  need = std::max(need, need2);
  if (!temp) {
    *temp_bytes = need;
    return hipSuccess;
  }
  e = rocprim::select(temp, need, keys_in, flags, keys_out, n_out, (size_t)n, stream);
  if (e != hipSuccess) return e;
  return rocprim::select(temp, need, vals_in, flags, vals_out, n_out, (size_t)n, stream);
}

hipError_t launch_build_windows(const uint8_t* residues, const uint64_t* offsets, uint32_t n_seq,
                                const int32_t* roles, int k, int end_exclusive, const uint8_t* lut,
                                uint64_t* keys, uint32_t* tags, uint32_t* alpha_flag,
                                hipStream_t stream) {
  const unsigned g = (unsigned)std::min<uint64_t>(8192, ((uint64_t)n_seq + 3) / 4);
  hipLaunchKernelGGL(build_windows_kernel, dim3(g ? g : 1), dim3(256), 0, stream, residues,
                     offsets, n_seq, roles, k, end_exclusive, lut, keys, tags, alpha_flag);
  return hipGetLastError();
}

hipError_t launch_signature_heads(const uint64_t* keys, uint64_t n, uint8_t* flags,
                                  uint32_t* head_idx, uint32_t* run, void* temp,
                                  size_t* temp_bytes, hipStream_t stream) {
  if (!temp)
    return rocprim::inclusive_scan(nullptr, *temp_bytes, head_idx, run, (size_t)n,
                                   rocprim::maximum<uint32_t>(), stream);
  hipLaunchKernelGGL(sig_heads_kernel, dim3(grid_for(n)), dim3(256), 0, stream, keys, n, flags,
                     head_idx);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return rocprim::inclusive_scan(temp, *temp_bytes, head_idx, run, (size_t)n,
                                 rocprim::maximum<uint32_t>(), stream);
}

hipError_t launch_signature_flags(const uint64_t* keys, const uint32_t* tags, uint64_t n,
                                  uint8_t* flags, uint32_t* head_idx, uint32_t* run, void* temp,
                                  size_t* temp_bytes, hipStream_t stream) {
  if (!temp)
    return rocprim::inclusive_scan(nullptr, *temp_bytes, head_idx, run, (size_t)n,
                                   rocprim::maximum<uint32_t>(), stream);
  hipLaunchKernelGGL(sig_heads_kernel, dim3(grid_for(n)), dim3(256), 0, stream, keys, n, flags,
                     head_idx);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = rocprim::inclusive_scan(temp, *temp_bytes, head_idx, run, (size_t)n,
                              rocprim::maximum<uint32_t>(), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sig_clear_kernel, dim3(grid_for(n)), dim3(256), 0, stream, keys, tags, run,
                     n, flags);
  return hipGetLastError();
}

}  // namespace kma
