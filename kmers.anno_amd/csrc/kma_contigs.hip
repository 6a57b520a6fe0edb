// kma_contigs.hip — the 6-frame contig path for CDNA4 (gfx950).
//
//   contigs_probe_quad_kernel  6-frame translation + window + probe + block compaction
//                      (KmerReference.java:157-203, KmerPosition.java:50-93)
//   contigs_group_scan_kernel / contigs_emit_kernel   canonical-order hit emission after a
//                      block-count scan
#include "../../include/kmeranno.h"
#include "kma_internal.h"
#include "kma_device.h"
#include "kma_tuning.h"

KMA_TUNING_BLOCK_CLOCK(kma_debug_block_clock_contigs)

namespace kma {
namespace {

// ---------------------------------------------------------------------------------------------
// 6-frame contig annotation. A block owns kContigTile consecutive forward positions x of the
// concatenated contigs. Position x anchors two windows whose DNA span is [x, x + 3K):
//   '+' : codons read forward at x, x+3, ..               (processKmers on getSequence)
//   '-' : reverse-complement codons, last codon first      (processKmers on getRSequence)
// Both have 1-based forward left edge x + 1 = KmerPosition.calcLeft. processKmers' end
// exclusion i < P_f - K works out to x + 3K + 3 <= len for '+' and 3 <= x <= len - 3K for '-'.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t contig_of(const uint64_t* __restrict__ off, uint32_t n,
                                              uint64_t g) {
  uint32_t lo = 0, hi = n;  // largest c with off[c] <= g
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint32_t base2(uint8_t c) {  // T,C,A,G -> 0..3; other -> 4
  switch (c | 0x20) {
    case 't': case 'u': return 0u;
    case 'c': return 1u;
    case 'a': return 2u;
    case 'g': return 3u;
    default: return 4u;
  }
}


// The two windows a position anchors ('+' and '-') are probed with the quad-cooperative bucket
// loads of the protein path (both probes' 8 dwordx4 of a lane in flight before any compare,
// DPP quad match); the tile's contigs are found once (two wave-parallel searches) and their
// offsets cached in LDS, so a position's contig costs no global loads. Hits are compacted per
// block in canonical order (position, '+' before '-'); group sums of the block counts and an emit
// pass (each block computes its offset from them) write every block's hits in order.
constexpr int kOffCache = 64;

// contig_of by a whole wave, 64 candidates per dependent load: the largest c < n with
// off[c] <= g (off[0] <= g), in ceil(log64 n) rounds (one for up to 64 contigs) instead of
// log2 n dependent loads by one lane. Offsets are non-decreasing, so the lanes whose candidate
// is <= g form a prefix.
__device__ __forceinline__ uint32_t contig_of_wave(const uint64_t* __restrict__ off, uint32_t n,
                                                   uint64_t g) {
  const uint32_t lane = threadIdx.x & 63;
  uint32_t lo = 0, span = n;  // the answer lies in [lo, lo + span)
  while (span > 1) {          // wave-uniform
    const uint32_t step = (span + 63) / 64;
    const uint32_t c = lo + lane * step;
    const bool le = lane * step < span && off[c] <= g;
    const uint32_t k = (uint32_t)__popcll(__ballot(le)) - 1u;  // lane 0's candidate is lo
    const uint32_t nlo = lo + k * step;
    span = min(step, lo + span - nlo);
    lo = nlo;
  }
  return lo;
}

// Waves per SIMD of the 6-frame probe: 8 with one slice per block (64 VGPRs); the sequential
// slices' loop carries a few more scalar and vector values (SGPR spills land in VGPR lanes) and
// takes 7 to stay clear of scratch.
constexpr int kContigOcc = kContigSeq > 1 ? 7 : 8;
template <int K, int M>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kContigOcc, 8))) void contigs_probe_quad_kernel(
    ContigArgs a) {
  // K > 8: a wide table (16-byte slots, kma_internal.h): one slot per lane of the quad.
  constexpr bool kWide = wide_k(K);
  constexpr int kS = kWide ? kWideSlots : kSlotsPerBucket;   // slots per bucket
  constexpr int kQ = kWide ? 4 : kBucketQuads;                // dwordx4 per bucket
  constexpr int kH = kWide ? 1 : kBucketHalves;               // 64-byte pieces per bucket
  constexpr int kSpan = kContigTile + 3 * K;
  __shared__ uint8_t bases[kSpan];
  __shared__ uint8_t aa_p[kSpan], aa_m[kSpan];
  __shared__ uint64_t offc[kOffCache + 1];
  __shared__ uint32_t crange[2];
  constexpr int CP = kContigPos * kContigSeq;  // slices of 256 positions per block
  __shared__ uint32_t wave_tot[kWavesPerBlock * CP];
  __shared__ uint8_t codon[64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, part = t & 3;
  // offsets[0] through the constant address space: a scalar load (every block reads it, so the
  // scalar cache serves it) in place of a vector round trip before the tile's DNA load
  const uint64_t base = ((const __attribute__((address_space(4))) uint64_t*)a.offsets)[0];
  const uint64_t end = base + a.total_bases;
  const uint64_t r0 = (uint64_t)blockIdx.x * kContigTile;
  const uint32_t nb = a.n_buckets;
  KMA_CLK(0);
  // The tile's DNA bytes: every load issued before the contig search below, so that their
  // round trip overlaps the offsets' (as a strided loop of load, wait, store they took three
  // dependent trips: ~3.8 us of a ~12 us block, profiles/r04/clock_c3_r04g.json).
  constexpr int kTileIters = (kSpan + 255) / 256;
  uint8_t tb[kTileIters];
#pragma unroll
  for (int j = 0; j < kTileIters; ++j) {
    const int i = t + 256 * j;
    const uint64_t g = base + r0 + i;
    tb[j] = i < kSpan && g < end ? a.dna[g] : (uint8_t)'N';
  }
  if (wave == 3) codon[lane] = a.codon_codes[lane];  // LDS copy of the kernel-argument table
  if (a.n_contig < (uint32_t)kOffCache) {
    // Every offset fits the cache: wave 0 loads them once and finds the tile's first / last
    // contig by ballot (the largest c with offsets[c] <= g is a prefix count; offsets[0] = base).
    if (wave == 0) {
      const uint32_t n = a.n_contig;
      const uint64_t last = r0 + kContigTile < a.total_bases ? r0 + kContigTile : a.total_bases;
      const uint64_t v = a.offsets[min((uint32_t)lane, n)];
      const uint32_t lo = (uint32_t)__popcll(__ballot((uint32_t)lane < n && v <= base + r0)) - 1u;
      const uint32_t hi =
          (uint32_t)__popcll(__ballot((uint32_t)lane < n && v <= base + last - 1)) - 1u;
      offc[lane] = __shfl(v, (int)min(lo + (uint32_t)lane, n), 64);  // offsets[min(lo + i, n)]
      const uint64_t vn = __shfl(v, (int)n, 64);
      if (lane == 0) {
        offc[kOffCache] = vn;
        crange[0] = lo;
        crange[1] = hi;
      }
    }
  } else if (wave < 2) {  // wave 0: the tile's first contig (and its offsets), wave 1: its last
    const uint64_t last = r0 + kContigTile < a.total_bases ? r0 + kContigTile : a.total_bases;
    const uint32_t c = contig_of_wave(a.offsets, a.n_contig, base + (wave ? last - 1 : r0));
    if (lane == 0) crange[wave] = c;
    if (wave == 0) {  // offsets c .. c + 64 (clamped): the tile's contigs if they are <= 64
      offc[lane] = a.offsets[min(c + lane, a.n_contig)];
      if (lane == 0) offc[kOffCache] = a.offsets[min(c + kOffCache, a.n_contig)];
    }
  }
#pragma unroll
  for (int j = 0; j < kTileIters; ++j) {
    const int i = t + 256 * j;
    if (i < kSpan) bases[i] = (uint8_t)(base + r0 + i < end ? base2(tb[j]) : 4u);
  }
  __syncthreads();
  KMA_CLK(1);  // tile loaded, contigs found
  const uint32_t c_lo = crange[0], nc = crange[1] - c_lo + 1;  // contigs meeting the tile
  for (int i = t; i < kSpan - 2; i += blockDim.x) {
    const uint32_t b0 = bases[i], b1 = bases[i + 1], b2 = bases[i + 2];
    if ((b0 | b1 | b2) & 4u) {
      aa_p[i] = aa_m[i] = 0;  // 'X'
    } else {
      aa_p[i] = codon[b0 * 16 + b1 * 4 + b2];
      aa_m[i] = codon[(b2 ^ 2u) * 16 + (b1 ^ 2u) * 4 + (b0 ^ 2u)];  // complement: x ^ 2
    }
  }
  __syncthreads();
  KMA_CLK(2);  // translated

  // Each lane owns positions tp + 256 h (h < kContigPos): both windows of every one of them are
  // probed with all their dwordx4 in flight before any compare. Quad q's member p takes
  // position 16 p + q of its wave (the lane permutation of kma_internal.h), so that one load
  // instruction covers 16 consecutive positions (same-frame windows 3 apart share minimizers,
  // hence lines); the results go back to position order through LDS before the compaction.
  constexpr int CL = kContigPos;  // positions per lane held at once (per sequential slice)
  const uint32_t tp = (uint32_t)(wave * 64 + 16 * (lane & 3) + (lane >> 2));
  // Contig, offset in it and its length of the tile's forward position tt (g < end).
  auto locate = [&](uint32_t tt, uint32_t& c, int64_t& x, int64_t& len) {
    const uint64_t g = base + r0 + tt;
    if (nc <= (uint32_t)kOffCache) {
      uint32_t lo = 0, hi = nc;  // largest i < nc with offc[i] <= g
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (offc[mid] <= g) lo = mid; else hi = mid;
      }
      c = c_lo + lo;
      x = (int64_t)(g - offc[lo]);
      len = (int64_t)(offc[lo + 1] - offc[lo]);
    } else {
      c = contig_of(a.offsets, a.n_contig, g);
      x = (int64_t)(g - a.offsets[c]);
      len = (int64_t)(a.offsets[c + 1] - a.offsets[c]);
    }
  };
  // Verdicts of every position go through LDS (fid + 1, 0 = no hit), lane t then takes position
  // t's (back to position order after the lane permutation) for the compaction.
  __shared__ uint32_t xv[CP][2][256];
#pragma unroll 1
  for (int sq = 0; sq < kContigSeq; ++sq) {
  uint32_t contig[CL];
  uint64_t key[CL][2];
  uint32_t bk[CL][2];
  bool ok[CL][2];
#pragma unroll
  for (int h = 0; h < CL; ++h) {
    const uint32_t tt = tp + 256u * (sq * CL + h);
    const uint64_t g = base + r0 + tt;
    contig[h] = c_lo;
    int64_t x = 0, len = 0;
    if (g < end) locate(tt, contig[h], x, len);
    bool pv = g < end && x + 3 * K + 3 <= len, mv = g < end && x >= 3 && x + 3 * K <= len;
    key[h][0] = key[h][1] = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const uint32_t cp = aa_p[tt + 3 * j], cm = aa_m[tt + 3 * j];
      pv = pv && cp != 0u;
      mv = mv && cm != 0u;
      key[h][0] = (key[h][0] << 5) | cp;
      key[h][1] |= (uint64_t)cm << (5 * j);
    }
    // invalid windows gather bucket 0 (one shared line; their verdicts are dropped)
    ok[h][0] = pv;
    ok[h][1] = mv;
    bk[h][0] = pv ? home_bucket(key[h][0], K, M, nb) : 0u;
    bk[h][1] = mv ? home_bucket(key[h][1], K, M, nb) : 0u;
  }
  uint4 q[CL][2][4][kH];  // every window's quad buckets: all dwordx4 in flight
  const uint4* lane_slots = reinterpret_cast<const uint4*>(a.slots) + part;
#pragma unroll
  for (int h = 0; h < CL; ++h)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint32_t b0 = quad_bcast<0>(bk[h][j]), b1 = quad_bcast<1>(bk[h][j]);
      const uint32_t b2 = quad_bcast<2>(bk[h][j]), b3 = quad_bcast<3>(bk[h][j]);
      const uint32_t bb[4] = {b0, b1, b2, b3};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint4* bp = lane_slots + (uint64_t)bb[r] * kQ;
#pragma unroll
        for (int hh = 0; hh < kH; ++hh) q[h][j][r][hh] = bp[4 * hh];
      }
    }
  KMA_CLK(3);  // bucket loads issued
#pragma unroll
  for (int h = 0; h < CL; ++h)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint32_t klo = (uint32_t)key[h][j];
      const uint32_t khi = kWide ? (uint32_t)(key[h][j] >> 32) : (uint32_t)(key[h][j] >> 32) << 24;
      const uint32_t need = filter_need<kS>(klo);
      uint32_t raw[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const uint32_t kl = rr == 0 ? quad_bcast<0>(klo) : rr == 1 ? quad_bcast<1>(klo)
                          : rr == 2 ? quad_bcast<2>(klo) : quad_bcast<3>(klo);
        const uint32_t kh = rr == 0 ? quad_bcast<0>(khi) : rr == 1 ? quad_bcast<1>(khi)
                          : rr == 2 ? quad_bcast<2>(khi) : quad_bcast<3>(khi);
        const uint32_t nd = rr == 0 ? quad_bcast<0>(need) : rr == 1 ? quad_bcast<1>(need)
                          : rr == 2 ? quad_bcast<2>(need) : quad_bcast<3>(need);
        if constexpr (kWide) raw[rr] = match_wide_raw(q[h][j][rr][0], kl, kh, nd, part);
        else raw[rr] = match_part_raw(q[h][j][rr], kl, kh, nd, part);
      }
      const uint32_t word = quad_reduce_scatter(raw, part);
      const uint32_t w = ok[h][j] ? word : 0u;
      bool hit = (w & kWordHit) != 0u;
      uint32_t fid = w & kFidMask;
      uint32_t sid = bk[h][j] * kS + ((w >> kSlotShift) & (kS - 1));
      if (ok[h][j] && w == 0u) {  // rare: home missed, every filter position set
        if constexpr (kWide)
          hit = walk_chain_wide(a.slots, nb, bk[h][j], key[h][j], fid, sid);
        else
          hit = walk_chain(a.slots, nb, bk[h][j], key[h][j], fid, sid, a.two_choice != 0);
      }
      if (a.strict_pass && hit) {  // KmerFactory.Strict: locations counted by slot id
        if (a.strict_pass == 1) atomicAdd(a.slot_count + sid, 1u);
        else hit = a.slot_count[sid] == 1u;
      }
      if (a.tally && hit && fid < a.n_fid)
        atomicAdd(a.tally + (uint64_t)contig[h] * a.n_fid + fid, 1u);
      xv[sq * CL + h][j][tp] = hit ? fid + 1u : 0u;
    }
  }  // sequential slices
  KMA_CLK(4);  // matched (chain walks done)
  __syncthreads();
  // Block-local compaction in canonical order (position, '+' before '-'): slice by slice, each
  // slice's verdicts read back from LDS twice (counts, then records) rather than kept live.
#pragma unroll 1
  for (int h = 0; h < CP; ++h) {
    const uint64_t bp = __ballot(xv[h][0][t] != 0u), bm = __ballot(xv[h][1][t] != 0u);
    if (lane == 0) wave_tot[h * kWavesPerBlock + wave] = (uint32_t)(__popcll(bp) + __popcll(bm));
  }
  __syncthreads();
  // Staged records are the final kma_hit (the emit pass only copies them): contig, left =
  // KmerPosition.calcLeft, fid, strand and frame (KmerPosition.java:50-93).
  uint32_t total = 0;
  uint4* st = reinterpret_cast<uint4*>(a.staging) + (uint64_t)blockIdx.x * (2 * kContigTile);
#pragma unroll 1
  for (int h = 0; h < CP; ++h) {
    const uint32_t v0 = xv[h][0][t], v1 = xv[h][1][t];
    const uint64_t bp = __ballot(v0 != 0u), bm = __ballot(v1 != 0u);
    uint32_t o = total + popc_below(bp) + popc_below(bm);
    for (int w = 0; w < kWavesPerBlock; ++w) {
      if (w < wave) o += wave_tot[h * kWavesPerBlock + w];
      total += wave_tot[h * kWavesPerBlock + w];
    }
    if (v0 | v1) {  // hits only at positions inside a contig (g < end)
      uint32_t c;
      int64_t x, len;
      locate(t + 256u * h, c, x, len);
      const uint32_t left = (uint32_t)(x + 1);
      if (v0) st[o++] = make_uint4(c, left, v0 - 1u, '+' | (uint32_t)(x % 3 + 1) << 8);
      if (v1) st[o] = make_uint4(c, left, v1 - 1u, '-' | (uint32_t)((len - 3 * K - x) % 3 + 1) << 8);
    }
  }
  if (t == 0) {
    a.block_counts[blockIdx.x] = total;
    // the emit pass's group sums (zeroed by the previous emit pass on this workspace)
    if (a.group_sum && total)
      __hip_atomic_fetch_add(a.group_sum + blockIdx.x / kScanGroup, (uint64_t)total,
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  KMA_CLK(5);
  KMA_CLK_HW();
}

// Exclusive prefix of block b's hit count (wave 0 of the emit block; wave-uniform result): the
// group sums of the groups before b's (kScanGroup probe blocks each, summed by the probe's
// atomics; every load issued at once: one round trip for up to 64 groups) — or, for calls of
// more than kDirectGroups groups, the exclusive group prefix contigs_group_scan_kernel left in
// place of the sums (one load) — plus the counts before b in its group.
__device__ __forceinline__ uint64_t emit_offset(const ContigArgs& a, uint32_t b) {
  const uint32_t lane = threadIdx.x & 63, g = b / kScanGroup;
  uint64_t s = 0;
  if (a.groups_scanned) {
    if (lane == 0) s = a.group_sum[g];
  } else {
    for (uint32_t i = lane; i < g; i += 64) s += a.group_sum[i];
  }
  const uint32_t c0 = g * kScanGroup + 4u * lane;  // counts are allocated in whole groups
  if (c0 < b) {
    const uint4 v = *reinterpret_cast<const uint4*>(a.block_counts + c0);
    s += (uint64_t)v.x + (c0 + 1 < b ? v.y : 0u) + (c0 + 2 < b ? v.z : 0u) +
         (c0 + 3 < b ? v.w : 0u);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  return s;
}

// Calls of more than kDirectGroups groups (> kDirectGroups x kScanGroup x kContigTile = 268M
// bases): one block turns the group sums into
// exclusive prefixes in place, so an emit block reads one value instead of summing every group
// before its own (which grows as blocks x groups: ~2e9 loads at 1 Gbp).
__global__ __launch_bounds__(1024) void contigs_group_scan_kernel(uint64_t* sums, uint32_t n) {
  __shared__ uint64_t part[1024];
  const uint32_t t = threadIdx.x, per = (n + 1023) / 1024;
  const uint64_t lo = (uint64_t)t * per, hi = lo + per < n ? lo + per : n;
  uint64_t s = 0;
  for (uint64_t i = lo; i < hi; ++i) s += sums[i];
  part[t] = s;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {  // inclusive Hillis-Steele scan of the parts
    const uint64_t v = t >= d ? part[t - d] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint64_t run = t ? part[t - 1] : 0u;
  for (uint64_t i = lo; i < hi; ++i) {
    const uint64_t x = sums[i];
    sums[i] = run;
    run += x;
  }
}

// Emit pass: an emit block takes kEmitSpan consecutive probe blocks; probe block b's staged
// records go to out[prefix[b] ..], those past `cap` are dropped; the last emit block publishes
// the total (the caller compares it with cap). The call leaves no state behind: every emit
// block counts itself done (one agent-scope atomic, issued once its offsets are read) and the
// block that finishes last zeroes the group sums and the counter for the next call (so calls
// on one workspace may be graph-captured and replayed). Measured alternatives for the offsets
// (c3, profiles/r03_ab/): a library two-kernel scan ~10 us; a ticket letting the probe's last
// block scan, 0.6 ms (20k atomics on one address serialize); a one-block scan kernel, ~18 us (a
// single CU's dependent round trips); a group-sum kernel between probe and emit, and one emit
// block per probe block (12.5 us for c3's 19.5k blocks of ~9 hits).
constexpr uint32_t kEmitSpan = 16;
__global__ __launch_bounds__(256) void contigs_emit_kernel(ContigArgs a, uint32_t n_blocks) {
  __shared__ uint64_t pre[kEmitSpan];
  __shared__ uint32_t cnt[kEmitSpan];
  __shared__ uint32_t last;
  const uint32_t b0 = blockIdx.x * kEmitSpan, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (wave == 0) {
    const uint32_t c = lane < kEmitSpan && b0 + lane < n_blocks ? a.block_counts[b0 + lane] : 0u;
    const uint64_t base = emit_offset(a, b0);
    uint64_t inc = c;  // inclusive scan over the span's counts (lanes < kEmitSpan)
#pragma unroll
    for (int d = 1; d < (int)kEmitSpan; d <<= 1) {
      const uint64_t v = __shfl_up(inc, d, 64);
      inc += lane >= (uint32_t)d ? v : 0u;
    }
    if (lane < kEmitSpan) {
      pre[lane] = base + inc - c;
      cnt[lane] = c;
    }
    if (blockIdx.x == gridDim.x - 1 && lane == kEmitSpan - 1) *a.n_hits = base + inc;
  }
  __syncthreads();
  // This block's reads of the group sums have returned (their values are in pre[], behind the
  // barrier), so a relaxed count suffices: the last block's zeroing cannot reach a read that
  // has already completed. (An acq_rel atomic here compiles to a whole-L2 writeback and
  // invalidate around it, buffer_wbl2 / buffer_inv, in every emit block: 18 vs ~5 us per c3
  // emit pass, profiles/r04_end/stats_c3_kernel_stats.csv.)
  if (t == 0)
    last = __hip_atomic_fetch_add(a.emit_done, 1u, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  // The span's records, flattened: thread t copies records t, t + 256, ... (kEmitU loads in
  // flight before their stores: no branch around a load, so the compiler keeps them in
  // registers and issues them back to back). Record r belongs to the last span block whose
  // first record is <= r. (A wave per probe block, a load-then-store loop per 64 records, took
  // a dependent round trip per iteration: 11.6 us per c3 emit pass, profiles/r04_final.)
  constexpr int kEmitU = 4;
  uint32_t first[kEmitSpan];  // span-local first record of each probe block
  const uint64_t p0 = pre[0];
#pragma unroll
  for (uint32_t k = 0; k < kEmitSpan; ++k) first[k] = (uint32_t)(pre[k] - p0);
  const uint32_t total = first[kEmitSpan - 1] + cnt[kEmitSpan - 1];
  const uint4* st = reinterpret_cast<const uint4*>(a.staging) + (uint64_t)b0 * (2 * kContigTile);
  uint4* out = reinterpret_cast<uint4*>(a.out);
  for (uint32_t r0 = 0; r0 < total; r0 += 256u * kEmitU) {
    uint4 v0, v1, v2, v3;
    uint32_t rr[kEmitU];
    uint64_t src[kEmitU];
#pragma unroll
    for (int u = 0; u < kEmitU; ++u) {
      const uint32_t r = r0 + 256u * u + t;
      rr[u] = r < total ? r : 0u;  // out of range: record 0 of the span (read, not stored)
      uint32_t i = 0, fi = 0;
#pragma unroll
      for (uint32_t k = 1; k < kEmitSpan; ++k)
        if (first[k] <= rr[u]) {
          i = k;
          fi = first[k];
        }
      src[u] = (uint64_t)i * (2 * kContigTile) + (rr[u] - fi);
    }
    v0 = st[src[0]];
    v1 = st[src[1]];
    v2 = st[src[2]];
    v3 = st[src[3]];
    const uint32_t r = r0 + t;
    if (r < total && p0 + r < a.cap) out[p0 + r] = v0;
    if (r + 256u < total && p0 + r + 256u < a.cap) out[p0 + r + 256u] = v1;
    if (r + 512u < total && p0 + r + 512u < a.cap) out[p0 + r + 512u] = v2;
    if (r + 768u < total && p0 + r + 768u < a.cap) out[p0 + r + 768u] = v3;
  }
  __syncthreads();
  if (last) {  // every other emit block has read its offsets: clean up for the next call
    for (uint32_t i = t; i < a.n_groups; i += 256) a.group_sum[i] = 0;
    if (t == 0) *a.emit_done = 0;
  }
}

}  // namespace

// ---- launchers ----------------------------------------------------------------------------------
template <int K, int M>
struct ContigLaunch {
  static hipError_t run(const ContigArgs& a, uint64_t n_blocks, hipStream_t stream) {
    hipLaunchKernelGGL((contigs_probe_quad_kernel<K, M>), dim3((unsigned)n_blocks), dim3(256), 0,
                       stream, a);
    return hipGetLastError();
  }
};

hipError_t launch_contigs_probe(const ContigArgs& a, uint64_t n_blocks, hipStream_t stream) {
  return dispatch_km<ContigLaunch>(a.k, a.mlen, a, n_blocks, stream);
}

hipError_t launch_contigs_emit(const ContigArgs& a, uint64_t n_blocks, hipStream_t stream) {
  ContigArgs e = a;
  e.n_groups = (uint32_t)((n_blocks + kScanGroup - 1) / kScanGroup);
  e.groups_scanned = e.n_groups > kDirectGroups;
  if (e.groups_scanned) {
    hipLaunchKernelGGL(contigs_group_scan_kernel, dim3(1), dim3(1024), 0, stream, e.group_sum,
                       e.n_groups);
    if (hipError_t err = hipGetLastError()) return err;
  }
  const unsigned g = (unsigned)((n_blocks + kEmitSpan - 1) / kEmitSpan);
  hipLaunchKernelGGL(contigs_emit_kernel, dim3(g), dim3(256), 0, stream, e, (uint32_t)n_blocks);
  return hipGetLastError();
}

}  // namespace kma
