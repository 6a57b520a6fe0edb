// kma_sigmerge.hip — the streamed signature build's kernels for CDNA4 (gfx950): the batch reduce
// (every key run of a sorted batch folded into one (key, state) row) and the union merge of the
// resident run with a reduced batch (a merge-path kernel: count pass, scan of the tiles' head
// counts, write pass). The state, its combine rule, the split search and the head rule are in
// kma_sigmerge.h, shared with the host check program.
#include <cstring>  // (rocprim.hpp uses memset without including it)
#include <rocprim/rocprim.hpp>

#include <algorithm>

#include "kma_internal.h"
#include "kma_device.h"
#include "kma_sigmerge.h"

namespace kma {
namespace {

// ---- batch reduce ---------------------------------------------------------------------------
// state[i] = the state of pair i alone (only the heads' entries are read afterwards).
__global__ __launch_bounds__(256) void sig_state_init_kernel(const uint32_t* __restrict__ tags,
                                                             uint64_t n,
                                                             uint32_t* __restrict__ state) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * 256)
    state[i] = sig_state_of_tag(tags[i], kBuildNeg);
}

// Every pair that is not its run's head raises the head's state to combine(head's own, its
// own): with role < kSigConflict < kSigBuffered the fold of a run is the largest of these (two
// roles differ somewhere in a run iff one differs from the head's), so an atomicMax per pair that
// changes anything does it; a run of one role issues none.
__global__ __launch_bounds__(256) void sig_fold_kernel(const uint64_t* __restrict__ k,
                                                       const uint32_t* __restrict__ tags,
                                                       const uint32_t* __restrict__ run,
                                                       uint64_t n, uint32_t* state) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * 256) {
    if (k[i] == 0) continue;
    const uint32_t h = run[i];
    if (h == (uint32_t)i) continue;
    const uint32_t hs = sig_state_of_tag(tags[h], kBuildNeg);
    const uint32_t v = sig_combine(hs, sig_state_of_tag(tags[i], kBuildNeg));
    if (v != hs) atomicMax(state + h, v);
  }
}

// ---- union merge ----------------------------------------------------------------------------
// A tile's split at diagonal d by one wave, 64 probes a step (kma_sigmerge.h sig_probe /
// sig_narrow); every lane returns the split.
__device__ __forceinline__ uint64_t wave_merge_split(const uint64_t* __restrict__ a, uint64_t nA,
                                                     const uint64_t* __restrict__ b, uint64_t nB,
                                                     uint64_t d, uint32_t lane) {
  uint64_t lo = sig_split_lo(nB, d), hi = sig_split_hi(nA, d);
  while (lo < hi) {  // (wave-uniform)
    const uint64_t m = sig_probe(lo, hi, lane);  // lo <= m < hi: m < nA and 0 <= d - 1 - m < nB
    const bool before = a[m] <= b[d - 1 - m];
    sig_narrow(&lo, &hi, (uint32_t)__popcll(__ballot(before)));
  }
  return lo;
}

// One block per tile of kSigTile merged positions. LDS: s_key[0] = A[i0 - 1] (0 when i0 == 0),
// then the tile's na keys of A, its nb keys of B and B[j1] (0 when j1 == nB); s_st alike.
// Thread t merges positions [8t, 8t + 8) of the tile from its own split in LDS. Count pass:
// tile_cnt[tile] = the tile's heads. Write pass: the heads' rows are packed in LDS and copied
// out in order from tile_off[tile].
template <bool Write>
__global__ __launch_bounds__(kSigBlock) void sig_merge_kernel(SigRun A, SigRun B,
                                                              uint64_t* __restrict__ tile_cnt,
                                                              const uint64_t* __restrict__ tile_off,
                                                              uint64_t* __restrict__ out_keys,
                                                              uint32_t* __restrict__ out_states) {
  __shared__ uint64_t s_key[kSigTile + 2];
  __shared__ uint32_t s_st[kSigTile + 2];
  __shared__ uint64_t s_split[2];
  __shared__ uint32_t s_wave[kSigBlock / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t nA = A.n, nB = B.n, total = nA + nB;
  const uint64_t tile = blockIdx.x;
  const uint64_t d0 = tile * kSigTile, d1 = std::min<uint64_t>(d0 + kSigTile, total);
  if (wave < 2) {
    const uint64_t i = wave_merge_split(A.keys, nA, B.keys, nB, wave ? d1 : d0, lane);
    if (lane == 0) s_split[wave] = i;
  }
  __syncthreads();
  const uint64_t i0 = s_split[0], i1 = s_split[1], j0 = d0 - i0, j1 = d1 - i1;
  const uint32_t na = (uint32_t)(i1 - i0), nb = (uint32_t)(j1 - j0), n = na + nb;
  uint64_t* const a = s_key + 1;
  uint64_t* const b = a + na;
  uint32_t* const sa = s_st + 1;
  uint32_t* const sb = sa + na;
  for (uint32_t x = tid; x < na; x += kSigBlock) {
    a[x] = A.keys[i0 + x];
    sa[x] = A.states[i0 + x];
  }
  for (uint32_t x = tid; x < nb; x += kSigBlock) {
    b[x] = B.keys[j0 + x];
    sb[x] = B.states[j0 + x];
  }
  if (tid == 0) {
    s_key[0] = i0 ? A.keys[i0 - 1] : 0;
    s_st[0] = 0;
    b[nb] = j1 < nB ? B.keys[j1] : 0;
    sb[nb] = j1 < nB ? B.states[j1] : 0;
  }
  __syncthreads();

  const uint32_t ld = std::min(tid * kSigPerThread, n);
  uint32_t ai = (uint32_t)sig_merge_split(a, na, b, nb, ld), bi = ld - ai;
  uint64_t key[kSigPerThread];
  uint32_t st[kSigPerThread];
  uint32_t heads = 0;  // bit e: position ld + e is a head
#pragma unroll
  for (uint32_t e = 0; e < kSigPerThread; ++e) {
    key[e] = 0;
    st[e] = 0;
    if (ld + e < n) {
      const uint64_t ka = a[ai], kb = b[bi];  // (a[na] is b[0], b[nb] the extra entry: in bounds)
      if (ai < na && sig_takes_a(ka, bi < nb, kb)) {
        const bool pair = sig_a_pairs(ka, j0 + bi < nB, kb);
        key[e] = ka;
        st[e] = pair ? sig_combine(sa[ai], sb[bi]) : sa[ai];
        heads |= 1u << e;
        ++ai;
      } else {
        key[e] = kb;
        st[e] = sb[bi];
        if (sig_b_is_head(i0 + ai > 0, a[(int)ai - 1], kb)) heads |= 1u << e;
        ++bi;
      }
    }
  }

  // the block's exclusive scan of the threads' head counts
  const uint32_t mine = (uint32_t)__popc(heads);
  uint32_t incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(incl, o, 64);
    if ((int)lane >= o) incl += v;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();  // (also: every thread is done reading s_key / s_st)
  uint32_t before = incl - mine, block_total = 0;
#pragma unroll
  for (uint32_t w = 0; w < kSigBlock / 64; ++w) {
    if (w < wave) before += s_wave[w];
    block_total += s_wave[w];
  }
  if (!Write) {
    if (tid == 0) {
      tile_cnt[tile] = block_total;
      if (tile == 0) tile_cnt[gridDim.x] = 0;  // the scan's last entry: the union's size
    }
    return;
  }
  uint32_t r = before;
#pragma unroll
  for (uint32_t e = 0; e < kSigPerThread; ++e)
    if (heads >> e & 1u) {
      s_key[r] = key[e];
      s_st[r] = st[e];
      ++r;
    }
  __syncthreads();
  const uint64_t base = tile_off[tile];
  for (uint32_t x = tid; x < block_total; x += kSigBlock) {
    out_keys[base + x] = s_key[x];
    out_states[base + x] = s_st[x];
  }
}

// ---- counts, finish -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sig_counts_kernel(const uint32_t* __restrict__ states,
                                                         uint64_t n, unsigned long long* counts) {
  uint32_t role = 0, conflict = 0, buffered = 0;  // (a thread sees < 2^32 states)
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * 256) {
    const uint32_t s = states[i];
    role += sig_is_role(s) ? 1u : 0u;
    conflict += s == kSigConflict ? 1u : 0u;
    buffered += s == kSigBuffered ? 1u : 0u;
  }
  role = wave_sum(role);
  conflict = wave_sum(conflict);
  buffered = wave_sum(buffered);
  if ((threadIdx.x & 63) == 0) {
    if (role) atomicAdd(counts + 0, (unsigned long long)role);
    if (conflict) atomicAdd(counts + 1, (unsigned long long)conflict);
    if (buffered) atomicAdd(counts + 2, (unsigned long long)buffered);
  }
}

__global__ __launch_bounds__(256) void sig_role_flags_kernel(const uint32_t* __restrict__ states,
                                                             uint64_t n,
                                                             uint8_t* __restrict__ flags) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * 256)
    flags[i] = sig_is_role(states[i]) ? 1 : 0;
}

unsigned grid_for(uint64_t n, unsigned cap = 8192) {
  const uint64_t g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace

hipError_t launch_sig_reduce(const uint64_t* keys, const uint32_t* tags, uint64_t n,
                             uint8_t* flags, uint32_t* head, uint32_t* run, uint64_t* out_keys,
                             uint32_t* out_states, uint64_t* d_n_out, void* temp,
                             size_t* temp_bytes, hipStream_t stream) {
  if (!temp) {
    size_t t1 = 0, t2 = 0;
    hipError_t e = launch_signature_heads(keys, n, flags, head, run, nullptr, &t1, stream);
    if (e != hipSuccess) return e;
    e = launch_select_flagged(nullptr, &t2, keys, head, flags, out_keys, out_states, d_n_out, n,
                              stream);
    *temp_bytes = std::max(t1, t2);
    return e;
  }
  size_t bytes = *temp_bytes;
  hipError_t e = launch_signature_heads(keys, n, flags, head, run, temp, &bytes, stream);
  if (e != hipSuccess) return e;
  uint32_t* state = head;  // the scan has consumed the head indices
  hipLaunchKernelGGL(sig_state_init_kernel, dim3(grid_for(n)), dim3(256), 0, stream, tags, n,
                     state);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(sig_fold_kernel, dim3(grid_for(n)), dim3(256), 0, stream, keys, tags, run, n,
                     state);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  bytes = *temp_bytes;
  return launch_select_flagged(temp, &bytes, keys, state, flags, out_keys, out_states, d_n_out, n,
                               stream);
}

hipError_t launch_sig_merge_count(const SigRun& a, const SigRun& b, uint64_t* tile_cnt,
                                  uint64_t* tile_off, void* temp, size_t* temp_bytes,
                                  hipStream_t stream) {
  const uint64_t n_tiles = sig_tiles(a.n, b.n, kSigTile);
  if (!temp)
    return rocprim::exclusive_scan(nullptr, *temp_bytes, tile_cnt, tile_off, (uint64_t)0,
                                   (size_t)(n_tiles + 1), rocprim::plus<uint64_t>(), stream);
  if (n_tiles == 0 || n_tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sig_merge_kernel<false>, dim3((unsigned)n_tiles), dim3(kSigBlock), 0, stream,
                     a, b, tile_cnt, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                     (uint32_t*)nullptr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return rocprim::exclusive_scan(temp, *temp_bytes, tile_cnt, tile_off, (uint64_t)0,
                                 (size_t)(n_tiles + 1), rocprim::plus<uint64_t>(), stream);
}

hipError_t launch_sig_merge_write(const SigRun& a, const SigRun& b, const uint64_t* tile_off,
                                  uint64_t* out_keys, uint32_t* out_states, hipStream_t stream) {
  const uint64_t n_tiles = sig_tiles(a.n, b.n, kSigTile);
  if (n_tiles == 0 || n_tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sig_merge_kernel<true>, dim3((unsigned)n_tiles), dim3(kSigBlock), 0, stream,
                     a, b, (uint64_t*)nullptr, tile_off, out_keys, out_states);
  return hipGetLastError();
}

hipError_t launch_sig_counts(const uint32_t* states, uint64_t n, unsigned long long* counts,
                             hipStream_t stream) {
  hipLaunchKernelGGL(sig_counts_kernel, dim3(grid_for(n, 2048)), dim3(256), 0, stream, states, n,
                     counts);
  return hipGetLastError();
}

hipError_t launch_sig_role_flags(const uint32_t* states, uint64_t n, uint8_t* flags,
                                 hipStream_t stream) {
  hipLaunchKernelGGL(sig_role_flags_kernel, dim3(grid_for(n)), dim3(256), 0, stream, states, n,
                     flags);
  return hipGetLastError();
}

}  // namespace kma
