// kma_md5.hip — MD5 digests of a resident residue batch, and the duplicate grouping of
// SequenceCheckProcessor (anno/SequenceCheckProcessor.java:92-133) over them.
//
//   md5_kernel     one wave per block, one lane per sequence at a time (kma_md5.h: Md5Lane). Every
//                  pass of the loop is one 64-byte block for every live lane, data and padding
//                  blocks alike (md5_build has no branch), so the 64 steps are issued once.
//                  Refill form (the default): a wave owns a contiguous range of sequences, cut by
//                  a search of the offsets so that ranges weigh about the same (bytes plus
//                  kMd5SeqWeight per sequence); a lane that ends a sequence stores its digest
//                  (one 16-byte store) and takes the range's next one by a ballot and
//                  popc_below. No global counter: nothing to reset, capturable in a graph.
//                  Static form (kMd5Static): lane i takes sequence 64 w + i; the wave runs as
//                  long as its longest sequence.
//                  Loads: each lane reads its own block as four 16-byte groups of aligned
//                  words, or (kMd5Coop) 16 lanes fetch one sequence's block, a dword each,
//                  through LDS: a load instruction then touches 4 sequences, not 64.
//   sc_* kernels   kma_check_sequences after the digests: (digest, index) sorted over all 128
//                  bits by two stable 64-bit rocPRIM radix sorts (low half, then high half),
//                  run heads, a max-scan that gives every position its run's head, and per
//                  run the member count and the minimum and maximum function id (atomics at
//                  the head). Stable sorts keep a run's members in input order: the head is
//                  the smallest index.
#include <cstring>  // (rocprim.hpp uses memset without including it)
#include <rocprim/rocprim.hpp>

#include "kma_device.h"
#include "kma_md5.h"

namespace kma {
namespace {

// The first sequence of wave w's range: the smallest s in [0, n_seq] whose weight (bytes before
// it + kMd5SeqWeight s) reaches w / n_waves of the batch's. Strictly increasing weights: cut(0)
// = 0, cut(n_waves) = n_seq. Wave-uniform.
__device__ __forceinline__ uint32_t md5_cut(const Md5Args& a, uint32_t w) {
  const uint64_t base = a.off[0];
  const uint64_t total = a.off[a.n_seq] - base + (uint64_t)kMd5SeqWeight * a.n_seq;
  const uint64_t target = total / a.n_waves * w + total % a.n_waves * w / a.n_waves;
  if (w == a.n_waves) return a.n_seq;
  uint32_t lo = 0, hi = a.n_seq;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a.off[mid] - base + (uint64_t)kMd5SeqWeight * mid >= target) hi = mid; else lo = mid + 1;
  }
  return lo;
}

constexpr uint32_t kStageStride = 17;  // words per lane in LDS: odd, so a lane's row reads spread

// The 16 words after each lane's q through LDS: in pass i lanes 16 j .. 16 j + 15 read the
// words of lane 4 i + j, each only where that lane needs it. All 64 lanes call it.
__device__ __forceinline__ void md5_coop_load(const Md5Lane& l, bool active, const uint8_t* res,
                                              uint32_t* stage, uint32_t lane, uint32_t (&w)[16]) {
  const uint32_t need = active ? l.words_needed() : 0u;
  // (as a byte offset from res, so that the reading lane's pointer is a global one)
  const uint64_t first =
      active ? (uint64_t)(reinterpret_cast<const uint8_t*>(l.q + 1) - res) : 0ull;
  const uint32_t k = lane & 15u;
#pragma unroll
  for (uint32_t i = 0; i < 16; ++i) {
    const uint32_t src = 4u * i + (lane >> 4);
    const uint64_t at = __shfl((unsigned long long)first, (int)src, 64);
    const uint32_t n = __shfl(need, (int)src, 64);
    uint32_t v = 0;
    if (k < n) v = reinterpret_cast<const uint32_t*>(res + at)[k];
    stage[src * kStageStride + k] = v;
  }
  __syncthreads();
#pragma unroll
  for (uint32_t i = 0; i < 16; ++i) w[i] = stage[lane * kStageStride + i];
  __syncthreads();
}

template <bool Upper, bool Refill, bool Coop>
__global__ __launch_bounds__(64) void md5_kernel(Md5Args a) {
  __shared__ uint32_t stage[Coop ? 64 * kStageStride : 1];
  const uint32_t lane = threadIdx.x;
  uint32_t s_lo, s_hi;
  if (Refill) {
    s_lo = md5_cut(a, blockIdx.x);
    s_hi = md5_cut(a, blockIdx.x + 1);
  } else {
    s_lo = blockIdx.x * 64u;  // (the grid is ceil(n_seq / 64): s_lo < n_seq)
    s_hi = a.n_seq - s_lo > 64u ? s_lo + 64u : a.n_seq;
  }
  uint64_t next = (uint64_t)s_lo + 64u;  // wave-uniform: the range's first sequence not taken
  uint32_t s = s_lo + lane;
  bool active = (uint64_t)s_lo + lane < s_hi;
  Md5Lane l;
  l.q = nullptr;
  l.sh = 0;
  l.rem = 0;
  if (active) l.begin(a.res, a.off[s], a.off[s + 1]);
  while (__ballot(active)) {
    uint32_t w[16];
    if (Coop) {
      md5_coop_load(l, active, a.res, stage, lane, w);
    } else if (active) {
      l.load(w);
    }
    bool done = false;
    if (active) {
      done = l.step<Upper>(w);
      if (done) a.digest[s] = make_uint4(l.h[0], l.h[1], l.h[2], l.h[3]);
    }
    if (Refill) {
      const uint64_t m = __ballot(done);
      if (done) {
        const uint64_t take = next + popc_below(m);
        active = take < s_hi;
        if (active) {
          s = (uint32_t)take;
          l.begin(a.res, a.off[s], a.off[s + 1]);
        }
      }
      next += (uint32_t)__popcll(m);
    } else if (done) {
      active = false;
    }
  }
}

template <bool Refill, bool Coop>
void md5_launch_form(const Md5Args& a, hipStream_t stream) {
  if (a.upper)
    hipLaunchKernelGGL((md5_kernel<true, Refill, Coop>), dim3(a.n_waves), dim3(64), 0, stream, a);
  else
    hipLaunchKernelGGL((md5_kernel<false, Refill, Coop>), dim3(a.n_waves), dim3(64), 0, stream, a);
}

// ---- grouping ----------------------------------------------------------------------------------
constexpr uint32_t kScBlock = 256;

__device__ __forceinline__ bool same_digest(const uint4& x, const uint4& y) {
  return x.x == y.x && x.y == y.y && x.z == y.z && x.w == y.w;
}

__global__ __launch_bounds__(kScBlock) void sc_low_keys(SeqCheckArgs a) {
  const uint32_t i = blockIdx.x * kScBlock + threadIdx.x;
  if (i >= a.n) return;
  const uint4 d = a.digest[i];
  a.key_a[i] = (uint64_t)d.y << 32 | d.x;
  a.idx_a[i] = i;
}

// After the first sort (idx_b in low-half order): the high halves in that order.
__global__ __launch_bounds__(kScBlock) void sc_high_keys(SeqCheckArgs a) {
  const uint32_t i = blockIdx.x * kScBlock + threadIdx.x;
  if (i >= a.n) return;
  const uint4 d = a.digest[a.idx_b[i]];
  a.key_a[i] = (uint64_t)d.w << 32 | d.z;
}

// After the second sort (idx_a in digest order): start[i] = i at a run's head, else 0, for the
// max-scan; the heads' accumulators cleared.
__global__ __launch_bounds__(kScBlock) void sc_heads(SeqCheckArgs a) {
  const uint32_t i = blockIdx.x * kScBlock + threadIdx.x;
  if (i >= a.n) return;
  const bool head = i == 0 || !same_digest(a.digest[a.idx_a[i]], a.digest[a.idx_a[i - 1]]);
  a.start[i] = head ? i : 0u;
  a.count[i] = 0u;
  a.fmin[i] = 0xFFFFFFFFu;
  a.fmax[i] = 0u;
}

__global__ __launch_bounds__(kScBlock) void sc_reduce(SeqCheckArgs a) {
  const uint32_t i = blockIdx.x * kScBlock + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t s = a.idx_a[i];
  if (a.off[s + 1] == a.off[s]) return;  // (the run of empty sequences counts nothing)
  const uint32_t st = a.start[i];
  atomicAdd(&a.count[st], 1u);
  if (a.fun) {
    const uint32_t f = a.fun[s];
    atomicMin(&a.fmin[st], f);
    atomicMax(&a.fmax[st], f);
  }
}

__global__ __launch_bounds__(kScBlock) void sc_emit(SeqCheckArgs a) {
  const uint32_t i = blockIdx.x * kScBlock + threadIdx.x;  // (whole waves reach the ballots)
  bool group = false, multi = false, bad = false;
  if (i < a.n) {
    const uint32_t s = a.idx_a[i];
    if (a.off[s + 1] == a.off[s]) {
      a.rep[s] = -1;
      a.size[s] = 0u;
      a.mixed[s] = 0;
    } else {
      const uint32_t st = a.start[i], c = a.count[st];
      const bool mix = a.fun && c > 1u && a.fmin[st] != a.fmax[st];
      a.rep[s] = (int32_t)a.idx_a[st];
      a.size[s] = c;
      a.mixed[s] = mix ? 1 : 0;
      group = i == st;
      multi = group && c > 1u;
      bad = group && mix;
    }
  }
  const uint64_t g = __ballot(group), m = __ballot(multi), b = __ballot(bad);
  if ((threadIdx.x & 63u) == 0u) {
    if (g) atomicAdd((unsigned long long*)&a.stats[0], (unsigned long long)__popcll(g));
    if (m) atomicAdd((unsigned long long*)&a.stats[1], (unsigned long long)__popcll(m));
    if (b) atomicAdd((unsigned long long*)&a.stats[2], (unsigned long long)__popcll(b));
  }
}

}  // namespace

uint32_t md5_waves(uint32_t n_seq, uint32_t form, uint32_t n_cu, uint32_t waves_per_cu) {
  const uint32_t full = (uint32_t)(((uint64_t)n_seq + 63u) / 64u);
  if (form & kMd5Static) return full;
  return std::max(1u, std::min(full, n_cu * (waves_per_cu ? waves_per_cu : kMd5Waves)));
}

hipError_t launch_md5(const Md5Args& a, uint32_t form, hipStream_t stream) {
  switch (form & (kMd5Static | kMd5Coop)) {
    case 0: md5_launch_form<true, false>(a, stream); break;
    case kMd5Static: md5_launch_form<false, false>(a, stream); break;
    case kMd5Coop: md5_launch_form<true, true>(a, stream); break;
    default: md5_launch_form<false, true>(a, stream); break;
  }
  return hipGetLastError();
}

hipError_t launch_seq_check(const SeqCheckArgs& a, void* temp, size_t* temp_bytes,
                            hipStream_t stream) {
  const size_t n = a.n;
  if (!temp) {
    size_t sort = 0, scan = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, sort, a.key_a, a.key_b, a.idx_a, a.idx_b, n,
                                             0u, 64u, stream);
    if (e != hipSuccess) return e;
    e = rocprim::inclusive_scan(nullptr, scan, a.start, a.start, n, rocprim::maximum<uint32_t>(),
                                stream);
    if (e != hipSuccess) return e;
    *temp_bytes = std::max(sort, scan);
    return hipSuccess;
  }
  const dim3 grid((unsigned)((n + kScBlock - 1) / kScBlock)), block(kScBlock);
  hipError_t e = hipMemsetAsync(a.stats, 0, 3 * sizeof(uint64_t), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sc_low_keys, grid, block, 0, stream, a);
  e = rocprim::radix_sort_pairs(temp, *temp_bytes, a.key_a, a.key_b, a.idx_a, a.idx_b, n, 0u, 64u,
                                stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sc_high_keys, grid, block, 0, stream, a);
  e = rocprim::radix_sort_pairs(temp, *temp_bytes, a.key_a, a.key_b, a.idx_b, a.idx_a, n, 0u, 64u,
                                stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sc_heads, grid, block, 0, stream, a);
  e = rocprim::inclusive_scan(temp, *temp_bytes, a.start, a.start, n,
                              rocprim::maximum<uint32_t>(), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sc_reduce, grid, block, 0, stream, a);
  hipLaunchKernelGGL(sc_emit, grid, block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace kma
