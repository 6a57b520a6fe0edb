// kma_kernels.hip — the protein probe for CDNA4 (gfx950), the hot path of signature-kmer
// annotation.
//
//   annotate_kernel    the protein path in one kernel: every window of every protein packed and
//                      probed in the table (the HashMap.get of ApplyKmerProcessor.java:130 for
//                      every kmer of ProteinKmers at :123), per-protein distinct-key sets and
//                      fid range in LDS, then the vote and min-hits threshold (:129-147).
//   pack_residues_kernel  ASCII residues -> the packed stream the stream kernels read.
//
// Table construction and the sort-and-scan builders are in kma_build.hip, the 6-frame path in
// kma_contigs.hip. Integer / byte work only: the bound is HBM (or Infinity-Cache) random access
// to 64-byte buckets, not MFMA.
#include <algorithm>

#include "../../include/kmeranno.h"
#include "kma_internal.h"
#include "kma_device.h"
#include "kma_tuning.h"

KMA_TUNING_BLOCK_CLOCK(kma_debug_block_clock)
KMA_TUNING_WALK_STATS(kma_debug_walk_stats)

namespace kma {
namespace {

// ---------------------------------------------------------------------------------------------
// The protein path (ApplyKmerProcessor.java:122-148 with ProteinKmers at :123): one kernel.
//
// A block owns kBlockProteins consecutive proteins. Every window of theirs is probed with
// quad-cooperative bucket loads: each lane packs its own windows' keys, then the four lanes of
// a quad read their four windows' buckets together (lane p loads bytes [16p, 16p + 16) of each:
// one wave instruction reads 16 whole 64-byte lines, the access shape with the higher measured
// random-gather rate) and combine matches with DPP quad ops. Adjacent lanes hold consecutive
// windows, which share their minimizer home bucket 1/3-1/2 of the time, so a repeated line is
// served by the CU's L1/L2 instead of HBM. Overflow chains (~1% of probes) are deferred to a
// per-wave LDS queue and walked 64 at a time.
//
// A hit updates its protein's record in LDS: smallest / largest fid (non-returning atomics)
// and the set of distinct keys hit (ProteinKmers is a set: a kmer occurring twice counts
// once; a key's slot id is its identity in the table). After one barrier the vote is read off
// the record, order-free: no hit -> NONE (roleId == null); smallest != largest -> AMBIGUOUS
// (badPeg); else the role with count = |set|, CALLED iff count >= minHits (:146).
//
// The Java loop breaks at the second role (:129, `!badPeg`), and so does the probe, a step at a
// time: an AMBIGUOUS protein reports fid -1 and count 0 and never reaches the tally, so a bucket
// line fetched for it once two fids are on record is a request the result does not use. At the
// top of every step each wave reads the block's records into a mask of its dead proteins
// (dead_mask); a dead protein's windows take the "does not probe" path (bucket 0, served from
// cache), its queued walks are dropped at flush time and its list is not deduplicated. The
// records only move apart, so a wave that sees a protein dead sees a fact that stays true, and
// one that sees it late only probes what it could have skipped: no synchronisation, and the
// outputs do not depend on timing because a dead protein's outputs are constants.
//
// Sets: ceil(1.5 x windows) u32 entries (load <= 2/3 however many windows hit) from the
// block's LDS pool, greedily in protein order; a protein that does not fit uses its own region
// of workspace memory (2 u32 per residue at its residues' offset), so any protein length is
// voted exactly. Windows that straddle two proteins are not probed.
// ---------------------------------------------------------------------------------------------

// Per-block protein records (LDS). The layout keeps kProteinOcc blocks per CU resident.
template <int P>
struct ProteinSmem {
  __attribute__((aligned(16))) uint32_t pool[kSetPool];  // LDS sets: slot id + 1, 0 = empty
  uint32_t chain_q[kWavesPerBlock][2 * kChainQ];  // deferred chain walks: packed key, protein
  uint32_t pbeg[P + 1];  // protein starts relative to the span start; [np..P] = span end
  uint32_t pwin[P];      // windows of the protein (ProteinKmers: L - K + 1, or L - K)
  uint32_t pset[P];      // set base in `pool`, or kGlobalSet
  uint32_t pcap[P];      // set capacity (0: no set)
  uint32_t pmin[P], pmax[P], pcnt[P];  // smallest / largest fid hit; distinct keys (or hits)
  uint32_t plist[P];                   // kGlobalSet proteins: hits appended to their list
  uint32_t skip;                       // two-pass grid: the group belongs to the other pass
  uint8_t lut[256];
};
static_assert(sizeof(ProteinSmem<kBlockProteins>) <= 163840 / kProteinOcc,
              "protein-path LDS must leave kProteinOcc blocks per CU");

// Insert slot id + 1 in a set of `cap` u32 entries; true if it was not there.
__device__ __forceinline__ bool lds_set_insert(uint32_t* set, uint32_t cap, uint32_t key) {
  uint32_t i = set_slot(key, cap);
  for (;;) {
    const uint32_t o = atomicCAS(set + i, 0u, key);
    if (o == 0u) return true;
    if (o == key) return false;
    i = i + 1 == cap ? 0u : i + 1;
  }
}
__device__ __forceinline__ bool global_set_insert(uint32_t* set, uint32_t cap, uint32_t key) {
  uint32_t i = set_slot(key, cap);
  for (;;) {
    uint32_t o = 0u;
    __hip_atomic_compare_exchange_strong(set + i, &o, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    if (o == 0u) return true;
    if (o == key) return false;
    i = i + 1 == cap ? 0u : i + 1;
  }
}

// A hit of protein p (of the block) on the key with slot id `sid` and function `fid`. A protein
// whose set is in LDS inserts the slot id there (a fresh key counts); a protein whose set did not
// fit (kGlobalSet) appends it to its list in workspace memory (its own residues' region: 2 u32
// per residue), deduplicated after the probe steps (dedupe_lists). Round 3 kept a hash set
// there, zeroed by the block and filled by agent-scope CAS: at c5 0.23 GB of writes per launch
// for 9 MB of outputs, the set lines being evicted from L2 between hits under the gather load.
template <int P>
__device__ __forceinline__ void record_hit(ProteinSmem<P>& sm, const ProteinArgs& a,
                                           uint64_t span_lo, bool multiset, uint32_t p,
                                           uint32_t fid, uint32_t sid) {
  atomicMin(&sm.pmin[p], fid);
  atomicMax(&sm.pmax[p], fid);
  bool fresh = true;  // multiset: every hit counts
  if (!multiset) {
    const uint32_t base = sm.pset[p];
    if (base != kGlobalSet) {
      fresh = lds_set_insert(sm.pool + base, sm.pcap[p], sid + 1u);
    } else {
      a.gset[2 * (span_lo + sm.pbeg[p]) + atomicAdd(&sm.plist[p], 1u)] = sid + 1u;
      fresh = false;
    }
  }
  if (fresh) atomicAdd(&sm.pcnt[p], 1u);
}

// The lane's index in its wave, computed where it is used: the probe loop of annotate_block has
// no register to carry it (or the thread index it comes from) across a step's bucket loads at
// 7 waves per SIMD, and the compiler spills such a value to scratch memory rather than compute
// it again. (volatile: not hoisted out of the loop, not merged with threadIdx.)
__device__ __forceinline__ uint32_t lane_id() {
  uint32_t lane;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
  return lane;
}

// After the probe steps (the LDS sets are final, the pool is free): the distinct slot ids of
// every kGlobalSet protein's list, counted into pcnt. A list of fewer than kSetPool hits is
// deduplicated in the pool (the usual case: it needs 2,730+ windows to have that many); a
// longer one (giant proteins) in a hash set of L entries in the second half of its region,
// zeroed here (agent-scope stores, the CAS inserts are agent-scope). The list of a protein that
// ended AMBIGUOUS is not read: its count is not reported. Block-uniform loop.
// (Protein bounds from LDS: indexing the kernel's register copy pb[] by the loop counter makes
// the compiler spill it to scratch.)
template <int P>
__device__ __forceinline__ void dedupe_lists(ProteinSmem<P>& sm, const ProteinArgs& a,
                                             uint64_t span_lo, const int t) {
  for (int p = 0; p < P; ++p) {
    if (sm.pset[p] != kGlobalSet) continue;
    if (sm.pmin[p] != sm.pmax[p]) continue;  // AMBIGUOUS (final here): its count is not reported
    const uint32_t h = sm.plist[p], b0 = sm.pbeg[p];
    if (h == 0) continue;
    const uint32_t* list = a.gset + 2 * (span_lo + b0);
    uint32_t fresh = 0;
    if (h < (uint32_t)kSetPool) {
      uint4* pool4 = reinterpret_cast<uint4*>(sm.pool);
      for (uint32_t i = t; i < (uint32_t)kSetPool / 4; i += 256) pool4[i] = make_uint4(0u, 0u, 0u, 0u);
      __syncthreads();
      for (uint32_t i = t; i < h; i += 256) fresh += lds_set_insert(sm.pool, kSetPool, list[i]);
    } else {
      const uint32_t L = sm.pbeg[p + 1] - b0;  // > windows >= h: the set never fills
      uint32_t* set = a.gset + 2 * (span_lo + b0) + L;
      for (uint32_t i = t; i < L; i += 256)
        __hip_atomic_store(set + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __threadfence();  // (giant proteins only: an L2 writeback per such protein)
      __syncthreads();
      for (uint32_t i = t; i < h; i += 256) fresh += global_set_insert(set, L, list[i]);
    }
    fresh = wave_sum(fresh);
    if ((t & 63) == 0 && fresh) atomicAdd(&sm.pcnt[p], fresh);
    __syncthreads();  // the pool (or the set) is free for the next list
  }
}

// The block's dead proteins, bit p for protein p: two different fids are on record, so the
// protein ends AMBIGUOUS whatever else it hits. Wave-uniform (a ballot: scalar registers).
// `mx > mn`, not `mn != mx`: a hit lowers pmin before it raises pmax, so a first hit seen
// between its two atomics reads mn = fid, mx = 0 (the initial value), which is no second fid.
// mx > mn >= 0 makes mx a recorded fid, and mn (below the initial 0xFFFFFFFF) another.
//
// The lane index comes from lane_id's mbcnt, which is not moved out of the step loop: a lane
// index (or the record's LDS address) held in a register across the step's bucket loads
// is one register more than the stream kernels have at 7 waves per SIMD (they spilled).
template <int P>
__device__ __forceinline__ uint32_t dead_mask(const ProteinSmem<P>& sm) {
  const uint32_t lane = lane_id();
  const uint32_t i = lane < (uint32_t)P ? lane : 0u;
  const uint32_t mn = sm.pmin[i], mx = sm.pmax[i];
  return (uint32_t)__ballot(lane < (uint32_t)P && mx > mn);
}

// Which of the block's proteins holds span position x (pb: the block-uniform starts, in
// scalar registers).
template <int P>
__device__ __forceinline__ uint32_t protein_at(const uint32_t (&pb)[P + 1], uint32_t x) {
  uint32_t p = 0;
#pragma unroll
  for (int i = 1; i < P; ++i) p += x >= pb[i] ? 1u : 0u;
  return p;
}
// Whether x (in protein p = protein_at(pb, x)) starts one of p's windows: pe[i] = pb[i] +
// windows of i <= pb[i + 1], so the proteins whose windows end at or below x are exactly those
// before p, plus p itself when x is past its last window. A compare count, like protein_at: a
// select of pe[p] is folded by the compiler into a dynamically indexed private array (scratch
// memory: 32 bytes per lane stored per block, ~2 GB of writes per c5 launch).
template <int P>
__device__ __forceinline__ bool window_at(const uint32_t (&pe)[P], uint32_t x, uint32_t p) {
  uint32_t ended = 0;
#pragma unroll
  for (int i = 0; i < P; ++i) ended += x >= pe[i] ? 1u : 0u;
  return ended == p;
}

// The lane's window within its wave's 64-position chunk: quad q's member p takes window
// 16 p + q (the lane permutation of kma_internal.h), so that load instruction r (member r of
// every quad) reads the buckets of 16 consecutive windows — windows that share a minimizer then
// share a line inside one instruction.
__device__ __forceinline__ uint32_t chunk_window(int t) {
  return (uint32_t)(16 * (t & 3) + ((t & 63) >> 2));
}
// The first span position of slot r's chunk in step s of a span of T steps (kma_internal.h).
__device__ __forceinline__ uint32_t chunk_pos(uint32_t r, uint32_t T, uint32_t s) {
  return 64u * (r * T + s);
}
// A wave-uniform value the compiler may not take apart: left to itself it splits a step's
// position `scalar(slot, step) + lane's window` into a loop-invariant vector register per
// window of the lane (slot part + lane's window) and a scalar step part, which is two registers
// more than the one lane's window, and the probe loop has none to spare at 7 waves per SIMD.
__device__ __forceinline__ uint32_t scalar_whole(uint32_t v) {
  asm volatile("" : "+s"(v));
  return v;
}

// A group's inputs that precede its first probe step: its proteins, the offsets wave 0 reads
// (lane <= np: offsets[p0 + lane]) and the span start: two dependent round trips with the
// first residues (offsets, then residues: 4.5 and ~4 us of a ~37 us c5 block at 6 proteins,
// profiles/r03_ab/r03o block clocks). A persistent grid loading the next group's head under
// the current group's steps was tried: the group loop cost 48-112 bytes per lane of register
// spills (scratch memory) at 7 waves per SIMD.
// xcd_group: block b -> group so that the blocks dispatched to one XCD (b mod 8, the
// round-robin dispatch) take consecutive groups: their offsets and span-edge residue lines
// then meet in that XCD's L2. A bijection on [0, n): the last n mod 8 blocks keep their index.
// Measured against block b taking group b (profiles/r03_session2/r03z_steps.log, arms
// interleaved): c5 3.618-3.631 vs 3.634-3.637 ms, c4 2.811 vs 2.824; c2 (two-pass grid) 2-7%
// slower, so not used there.
__device__ __forceinline__ uint32_t xcd_group(uint32_t b, uint32_t n) {
  const uint32_t per = n >> 3;
  return b < 8u * per ? (b & 7u) * per + (b >> 3) : b;
}

struct GroupHead {
  uint32_t p0, np;
  uint32_t steps;  // T: the span's probe steps (the step order needs it for the first residues)
  uint64_t beg_raw;
  uint64_t span_lo;
};
__device__ __forceinline__ void head_offsets(const ProteinArgs& a, uint32_t g, GroupHead& h) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  h.p0 = g * a.block_proteins;  // g < n_groups: p0 < n_seq
  h.np = min(a.block_proteins, a.n_seq - h.p0);
  h.beg_raw = wave == 0 && lane <= (int)h.np ? a.offsets[h.p0 + lane] : 0u;
  // (both ends of the span: block-uniform loads issued together, no further round trip)
  const uint64_t lo = a.offsets[h.p0], hi = a.offsets[h.p0 + h.np];
  h.span_lo = lo - a.offsets[0];
  h.steps = (uint32_t)((hi - lo + 256u * kProbeWin - 1u) / (256u * kProbeWin));
}
// Window x of the span is at position x + pos0 of `res`. ASCII residues: `res` is the aligned
// word at or below the span's first byte (d_residues is 8-byte aligned) and pos0 < 8 the byte
// offset; packed streams (Packed): `res` is the stream and pos0 the span's first residue in it
// (the stream starts at the call's first residue).
template <bool Packed>
__device__ __forceinline__ const uint8_t* head_res(const ProteinArgs& a, const GroupHead& h,
                                                   uint64_t& pos0) {
  if (Packed) {
    pos0 = a.stream_first + h.span_lo;
    return a.residues;
  }
  const uint8_t* res0 = a.residues + a.offsets[0] + h.span_lo;
  pos0 = (uintptr_t)res0 & 7u;
  return res0 - pos0;
}
// The group's first probe step's stream words (clamped to the batch, which is readable past
// its end; windows past the span are masked in the loop).
template <int U>
__device__ __forceinline__ void head_residues(const ProteinArgs& a, const GroupHead& h,
                                              uint32_t wave, uint32_t cw, WinWords (&ww)[U]) {
  uint64_t pos0;
  const uint8_t* res = head_res<true>(a, h, pos0);
  const uint64_t lim = a.n_residues - h.span_lo;
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const uint32_t x = chunk_pos(kWavesPerBlock * j + wave, h.steps, 0u) + cw;
    ww[j] = window_words_packed(res, (x < lim ? x : 0u) + pos0);
  }
}

// The ASCII kernel's stage (kma_internal.h) for steps s, s + 1 (s even) of a span of T steps: the
// block's thread t takes the 8-residue groups t, t + 256, .. of the stage. Group g is group
// g % kRegionGroups of slot g / kRegionGroups' region: the span's residues [x, x + 8) from
// stage_group_pos (a multiple of 8, so one funnel shift serves every group): the two aligned
// words around them, funnelled as a window's bytes are (`res` and `sh` from head_res<false>).
// Only groups that start below `lim` (the span's length, or what is left of the batch while the
// span is not known yet) are read, so the last word read is the one the last window's own ASCII
// load would read; the others (the regions of slots whose chunks lie past the span among them)
// read the span's first words and are stored as zero groups. The words wait in the lane's
// window registers ww[i].lo / .hi, which are free between a step's keys and the next step's
// windows: registers of their own spilled at 7 waves per SIMD.
constexpr int kStagePerThread = (kStageGroups + 255) / 256;
static_assert(kStagePerThread <= kProbeWin, "a lane's stage words wait in its window registers");
__device__ __forceinline__ uint32_t stage_group_pos(uint32_t g, uint32_t T, uint32_t s) {
  const uint32_t r = g / (uint32_t)kRegionGroups;
  return chunk_pos(r, T, s) + 8u * (g - r * (uint32_t)kRegionGroups);
}
__device__ __forceinline__ void stage_fetch(const uint8_t* __restrict__ res, uint32_t T,
                                            uint32_t s, uint32_t lim, WinWords (&ww)[kProbeWin]) {
  const uint64_t* words = reinterpret_cast<const uint64_t*>(res);
#pragma unroll
  for (int i = 0; i < kStagePerThread; ++i) {
    const uint32_t g = threadIdx.x + 256u * i;
    const uint32_t x = stage_group_pos(g, T, s);
    const bool in = g < (uint32_t)kStageGroups && x < lim;
    const uint64_t* src = words + (in ? x >> 3 : 0u);
    ww[i].lo = src[0];
    ww[i].hi = src[1];
  }
}
__device__ __forceinline__ void stage_store(uint8_t* stage, const uint8_t* lut, uint32_t sh,
                                            uint32_t T, uint32_t s, uint32_t lim,
                                            const WinWords (&ww)[kProbeWin]) {
#pragma unroll
  for (int i = 0; i < kStagePerThread; ++i) {
    const uint32_t g = threadIdx.x + 256u * i;
    if (g < (uint32_t)kStageGroups) {
      const bool in = stage_group_pos(g, T, s) < lim;
      store40(stage + 5u * g, in ? pack8(lut, funnel(ww[i].lo, ww[i].hi, sh)) : 0u);
    }
  }
}

// The group h: proteins [p0, p0 + np) (np <= P), contiguous in the batch, whose first step's
// stream words (Packed) or first stage's residue words (ASCII, stage_fetch) are in ww. pass
// 0 / 1: a block of the two-pass grid, which annotates its group only if the group is long
// (pass 0) / short (pass 1: fewer than defer_below probe steps); pass -1: always. sm.lut is
// being loaded (read after the first barrier).
//
// Step order (kma_internal.h): the span's T = h.steps steps each take one 64-position chunk per
// slot r = kWavesPerBlock j + wave, chunk r T + s in step s, so a step samples the whole span
// and the dead mask at the top of a step spares a protein that turned AMBIGUOUS the windows
// every slot still has ahead of it. Inside a chunk, and in everything indexed by the span
// position x, nothing depends on the order.
//
// ASCII residues (!Packed) are packed into the stage, the last kStageEntries entries of the
// pool (the sets take the rest), and every window then reads its key from there exactly as the
// packed kernel reads it from the stream: two 8-byte LDS reads and a funnel. The first stage
// is stored between the prologue's barriers; a span of more than kStageSteps steps stores the
// next one every kStageSteps steps between two block barriers of its own (the loop's bounds
// are block-uniform).
template <int K, int M, int P, bool Packed>
__device__ __forceinline__ void annotate_block(const ProteinArgs& a, ProteinSmem<P>& sm,
                                               const GroupHead& h, WinWords (&ww)[kProbeWin],
                                               const int pass = -1) {
  constexpr uint32_t kPool = Packed ? kSetPool : kSetPool - kStageEntries;  // entries for sets
  constexpr int U = kProbeWin;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, part = t & 3;
  const bool multiset = (a.flags & KMA_F_MULTISET) != 0;
  const uint32_t T = h.steps;
  // A window's position is chunk_pos(kWavesPerBlock j + wv, T, s) + cw: a scalar and the lane's
  // one register. The ASCII kernel needs the lane's window by itself for the stage, so its
  // wave's term is in the scalar (wv: the wave, in a scalar register); the stream kernels put
  // it into the lane's register, as the position had it before the strided order (wv = 0): they
  // are the first to spill.
  const uint32_t ws = (uint32_t)__builtin_amdgcn_readfirstlane(wave);
  const uint32_t wv = Packed ? 0u : ws;
  const uint32_t cw = chunk_window(t) + (Packed ? chunk_pos((uint32_t)wave, T, 0u) : 0u);
  const uint32_t p0 = h.p0, np = h.np;
  const uint64_t beg_raw = h.beg_raw, span_lo = h.span_lo;
  const uint64_t o0 = a.offsets[0];
  uint64_t pos0;
  const uint8_t* __restrict__ res = head_res<Packed>(a, h, pos0);
  if (wave == 0) {  // the block's protein records
    const uint64_t beg = lane <= (int)np ? beg_raw - o0 : 0u;
    const uint64_t end = __shfl_down(beg, 1, 64);
    const uint64_t lo = __shfl(beg, 0, 64), span_end = __shfl(beg, (int)np, 64);
    if (pass >= 0 && lane == 0) {  // two-pass grid: is the group this pass's?
      const bool short_group = span_end - lo < (uint64_t)a.defer_below * 256u * kProbeWin;
      sm.skip = short_group != (pass == 1) ? 1u : 0u;
    }
    if (lane <= P) sm.pbeg[lane] = (uint32_t)((lane <= (int)np ? beg : span_end) - lo);
    if (lane < P) {
      uint32_t nw = 0;
      if (lane < (int)np) {
        const int64_t n = (int64_t)(end - beg) - K + ((a.flags & KMA_F_END_EXCLUSIVE) ? 0 : 1);
        nw = n > 0 ? (uint32_t)n : 0u;
      }
      sm.pwin[lane] = nw;
      sm.pcap[lane] = (nw == 0 || multiset) ? 0u : ((nw + (nw >> 1) + 4u) & ~3u);
      sm.pmin[lane] = 0xFFFFFFFFu;
      sm.pmax[lane] = 0u;
      sm.pcnt[lane] = 0u;
      sm.plist[lane] = 0u;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {  // LDS pool for the sets; workspace memory for those that do not fit
      uint32_t sum = 0;
      for (int p = 0; p < P; ++p) sum += sm.pcap[p];
      uint32_t top = 0;
      if (sum <= kPool) {  // the usual case: every set in LDS, in protein order
        for (int p = 0; p < P; ++p) {
          sm.pset[p] = top;
          top += sm.pcap[p];
        }
      } else {
        // First fit by decreasing size (fewer windows left to workspace sets than protein
        // order: 1.9% vs 2.4% of c5's windows in a simulation of its length distribution).
        uint32_t done = 0;
        for (int it = 0; it < P; ++it) {
          int best = -1;
          for (int p = 0; p < P; ++p)
            if (!(done >> p & 1u) && (best < 0 || sm.pcap[p] > sm.pcap[best])) best = p;
          done |= 1u << best;
          const uint32_t cap = sm.pcap[best];
          const bool fits = top + cap <= kPool;
          sm.pset[best] = fits ? top : kGlobalSet;  // (a list: appended, never zeroed)
          top += fits ? cap : 0u;
        }
      }
      sm.chain_q[0][0] = top;  // pool entries in use (read before the queues are)
    }
  }
  __syncthreads();
  if (pass >= 0 && sm.skip) return;  // block-uniform
  uint8_t* stage = reinterpret_cast<uint8_t*>(sm.pool + kPool);
  const uint32_t stage_sh = (uint32_t)pos0 * 8u;
  // the first stage: beside the zeroing of the sets below it, read after the third barrier
  if (!Packed) stage_store(stage, sm.lut, stage_sh, T, 0u, a.n_residues - (uint32_t)span_lo, ww);
  const uint32_t used = sm.chain_q[0][0];
  uint32_t pb[P + 1], pe[P];
#pragma unroll
  for (int i = 0; i <= P; ++i) pb[i] = __builtin_amdgcn_readfirstlane(sm.pbeg[i]);
#pragma unroll
  for (int i = 0; i < P; ++i) pe[i] = __builtin_amdgcn_readfirstlane(sm.pbeg[i] + sm.pwin[i]);
  const uint32_t span = pb[P];
  __syncthreads();  // `used` has been read by every wave
  uint4* pool4 = reinterpret_cast<uint4*>(sm.pool);
  KMA_CLK(1);
  for (uint32_t i = t; i < used / 4; i += 256) pool4[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();

  const uint64_t* __restrict__ slots = a.slots;
  const uint32_t nb = a.n_buckets;
  const bool two_choice = a.two_choice != 0;
  uint32_t* cq = sm.chain_q[ws];
  uint32_t cn = 0;  // wave-uniform queue length
  // Deferred chain walks, 64 queued windows at a time: lane (quad g, member p) takes entry
  // 16 p + g of the chunk; the chain's first bucket of every entry is loaded and matched by a
  // quad (the probe loop's cooperative loads: 2 line requests per bucket instead of 8 dwordx4
  // of one lane), and only an entry whose first chain bucket is full and misses walks on alone.
  // Deferred chain walks: one lane per queued window (its packed key and protein from the
  // queue), whole-bucket loads. Measured against alternatives at c5 (profiles/r03_ab): queueing
  // positions and re-packing the residues 3.955 vs 3.86 ms; the chain's first bucket matched by
  // quads with cooperative loads 4.01 vs 3.94 ms (6.31 vs 6.35 at load factor 0.9).
  auto chain_flush = [&]() {
    __builtin_amdgcn_wave_barrier();  // queue writes of other lanes are visible (LDS in order)
    KMA_COUNT(0, 1);
    KMA_COUNT(1, cn);
    KMA_IF_COUNT(uint32_t wsum = 0, wmax = 0;)
    const uint32_t dead_now = dead_mask<P>(sm);  // (a later look than the entries' own steps')
    for (uint32_t e = lane_id(); e < cn; e += 64) {
      const uint32_t w2 = cq[2 * e + 1];
      const uint64_t key = (uint64_t)(w2 & 0xFFu) << 32 | cq[2 * e];
      const uint32_t p = w2 >> 8;
      if (dead_now >> p & 1u) continue;  // no alternate bucket is requested for a dead protein
      uint32_t fid = 0, sid = 0;
      KMA_IF_COUNT(uint32_t walked = 0;)
      const bool hit = walk_chain(slots, nb, home_bucket(key, K, M, nb), key, fid, sid, two_choice
                                  KMA_COUNT_ARG(&walked));
      if (hit) record_hit<P>(sm, a, span_lo, multiset, p, fid, sid);
      KMA_IF_COUNT(const uint32_t s1 = chain_bucket(home_bucket(key, K, M, nb), 1u, nb);)
      KMA_IF_COUNT(const bool first = hit && sid / kSlotsPerBucket == s1;)  // in chain step 1
      KMA_COUNT(4, __popcll(__ballot(hit)));
      KMA_COUNT(5, __popcll(__ballot(first)));
      KMA_IF_COUNT(wsum += walked; wmax = walked > wmax ? walked : wmax;)
    }
    KMA_COUNT(6, wave_sum(wsum));  // chain buckets loaded by walks (converged here)
    KMA_COUNT(7, wave_max(wmax));  // the flush waits for its longest walk
    __builtin_amdgcn_wave_barrier();
    cn = 0;
  };
  // A step's windows: packed keys (khi: key bits 32..39 << 24, bit 0 set for a window that
  // does not probe; the match reads khi's top byte only), filter masks and home buckets (bk:
  // protein << kBucketBits | home bucket, bucket 0 for a window that does not probe), from the
  // residues in ww. (A kNone sentinel in bk cost the gather a compare and a select per bucket;
  // a separate flag array, SGPR spills in the ASCII kernels.)
  struct Prep {
    uint32_t klo[U], khi[U], need[U], bk[U];
  };
  auto prep = [&](uint32_t s, Prep& o) {
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const uint32_t xc = chunk_pos(kWavesPerBlock * j + wv, T, s);
      const uint32_t x = (Packed ? xc : scalar_whole(xc)) + cw;
      const uint32_t p = protein_at<P>(pb, x);
      // (key 0: every residue without a code; it would match an empty slot)
      const uint64_t key = packed_key<K>(ww[j]);
      const bool ok = key != 0 && x < span && window_at<P>(pe, x, p);
      o.klo[j] = (uint32_t)key;
      o.khi[j] = (uint32_t)(key >> 32) << 24 | (ok ? 0u : 1u);  // bit 0: does not probe
      o.need[j] = filter_need<kSlotsPerBucket>(o.klo[j]);
      o.bk[j] = p << kBucketBits | (ok ? home_bucket(key, K, M, nb) : 0u);
    }
  };
  // Cooperative loads: the quad's four buckets, 64 bytes at a time (lane `part` reads bytes
  // [16 part, 16 part + 16) of each 64-byte half), all dwordx4 of the lane in flight before any
  // compare. A window that does not probe reads bucket 0 (result discarded).
  auto gather = [&](const Prep& c, uint4 (&q)[U][4][kBucketHalves]) {
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const uint32_t b0 = quad_bcast<0>(c.bk[j]), b1 = quad_bcast<1>(c.bk[j]);
      const uint32_t b2 = quad_bcast<2>(c.bk[j]), b3 = quad_bcast<3>(c.bk[j]);
      const uint32_t bb[4] = {b0, b1, b2, b3};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint4* bp = reinterpret_cast<const uint4*>(slots) + part +
                          (uint64_t)(bb[r] & kBucketIdx) * kBucketQuads;
#pragma unroll
        for (int h = 0; h < kBucketHalves; ++h) q[j][r][h] = bp[4 * h];
      }
    }
  };
  auto load_residues = [&](uint32_t s) {
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const uint32_t r = kWavesPerBlock * j + wv;
      if (Packed) {
        const uint32_t x = chunk_pos(r, T, s) + cw;
        ww[j] = window_words_packed(res, (x < span ? x : 0u) + pos0);
      } else {  // (s's stage is the one in LDS; a step past the span reads stale groups, masked)
        const uint32_t at = (uint32_t)kRegionRes * r + 64u * (s % (uint32_t)kStageSteps);
        ww[j] = window_words_packed(stage, scalar_whole(at) + cw);
      }
    }
  };
  // Compare the quad's buckets, record hits, queue chain walks.
  auto settle = [&](const Prep& c, const uint4 (&q)[U][4][kBucketHalves]) {
    uint32_t word[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      word[j] = 0;
      uint32_t raw[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t kl = r == 0 ? quad_bcast<0>(c.klo[j]) : r == 1 ? quad_bcast<1>(c.klo[j])
                          : r == 2 ? quad_bcast<2>(c.klo[j]) : quad_bcast<3>(c.klo[j]);
        const uint32_t kh = r == 0 ? quad_bcast<0>(c.khi[j]) : r == 1 ? quad_bcast<1>(c.khi[j])
                          : r == 2 ? quad_bcast<2>(c.khi[j]) : quad_bcast<3>(c.khi[j]);
        const uint32_t nd = r == 0 ? quad_bcast<0>(c.need[j]) : r == 1 ? quad_bcast<1>(c.need[j])
                          : r == 2 ? quad_bcast<2>(c.need[j]) : quad_bcast<3>(c.need[j]);
        raw[r] = match_part_raw(q[j][r], kl, kh, nd, part);
      }
      word[j] = quad_reduce_scatter(raw, part);
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const bool probed = (c.khi[j] & 1u) == 0u;
      const uint32_t w = probed ? word[j] : 0u;
      KMA_COUNT(2, __popcll(__ballot(probed)));
      KMA_COUNT(3, __popcll(__ballot((w & kWordHit) != 0u)));
      if (w & kWordHit)
        record_hit<P>(sm, a, span_lo, multiset, c.bk[j] >> kBucketBits, w & kFidMask,
                      (c.bk[j] & kBucketIdx) * kSlotsPerBucket + ((w >> kSlotShift) & kSlotMask));
      // rare: the home bucket missed and the key's filter positions are set -> deferred walk
      // (never for a protein dead at the top of the step: its windows are not `probed`)
      const bool pend = probed && w == 0u;
      const uint64_t m = __ballot(pend);
      if (pend) {  // queue entry: key bits 0..31; key bits 32..39 | protein << 8
        const uint32_t e = cn + popc_below(m);
        cq[2 * e] = c.klo[j];
        cq[2 * e + 1] = (c.khi[j] >> 24) | (c.bk[j] >> kBucketBits) << 8;
      }
      cn += (uint32_t)__popcll(m);
    }
    if (cn > (uint32_t)(kChainQ - 64 * U)) chain_flush();
  };
  // Software pipeline: the residues of step i + 1 are loaded while step i's buckets are in
  // flight, so a wave's only exposed latency per step is the bucket gather. (A two-stage
  // pipeline packing step i + 1 under step i's gather measured 6.51 vs 4.48 ms at c5,
  // profiles/r03_ab/r03h_steps.log.)
  if (!Packed) load_residues(0u);
  for (uint32_t s = 0; s < T; ++s) {
    // A protein dead by now (dead_mask) has no windows from here on: pe[i] = pb[i] makes
    // window_at false for every x of protein i and changes it for no other x (x of a later
    // protein is >= both, x of an earlier one below both), so the skip costs a window nothing:
    // it takes the "does not probe" path of prep. Scalar selects, no register of its own.
    const uint32_t dead = dead_mask<P>(sm);
#pragma unroll
    for (int i = 0; i < P; ++i) pe[i] = dead >> i & 1u ? pb[i] : pe[i];
    Prep cur;
    prep(s, cur);
    // The next step opens a new stage: its residue words are requested ahead of the bucket
    // loads and stored under them. Every wave has taken this step's windows from the old stage
    // once it is past prep, hence the first barrier. (Stored after settle instead: c5 2.768 vs
    // 2.751 ms)
    const uint32_t sn = s + 1u;
    const bool restage = !Packed && sn % (uint32_t)kStageSteps == 0u && sn < T;  // block-uniform
    if (restage) stage_fetch(res, T, sn, span, ww);
    uint4 q[U][4][kBucketHalves];
    gather(cur, q);
    // next step's residues (issued after the bucket loads: waiting for those leaves these in
    // flight, vmcnt counts in order)
    if (Packed) load_residues(sn);  // (past the span: clamped to its first word)
    if (restage) {  // (under the bucket loads: its words arrive first, the barriers wait with them)
      __syncthreads();
      stage_store(stage, sm.lut, stage_sh, T, sn, span, ww);
      __syncthreads();
    }
    settle(cur, q);
    // (from the stage: an LDS round trip, not worth ten registers held across the buckets)
    if (!Packed) load_residues(sn);
    if (s == 0) KMA_CLK(2);
  }
  KMA_CLK(3);
  KMA_CLK_SET(7, T);
  if (cn) chain_flush();
  KMA_CLK(4);
  __syncthreads();  // every LDS set is final; the lists are complete
  // (the thread index again, from the wave and the lane: see lane_id)
  const int te = (int)(64u * ws + lane_id());
  if (!multiset) dedupe_lists<P>(sm, a, span_lo, te);
  if (te < (int)np) {
    const int t = te;
    const uint32_t mn = sm.pmin[t], mx = sm.pmax[t], cnt = sm.pcnt[t];
    int32_t fid_out = -1, cnt_out = 0;
    uint8_t st;
    if (mn == 0xFFFFFFFFu) {
      st = KMA_STATUS_NONE;  // roleId == null
    } else if (mn != mx) {
      st = KMA_STATUS_AMBIGUOUS;  // badPeg
    } else {
      fid_out = (int32_t)mn;
      cnt_out = (int32_t)cnt;
      st = cnt >= (uint32_t)a.min_hits ? KMA_STATUS_CALLED : KMA_STATUS_BELOW_MIN;
      if (st == KMA_STATUS_CALLED && a.tally && mn < a.n_fid) atomicAdd(a.tally + mn, 1u);
    }
    a.out_fid[p0 + t] = fid_out;
    a.out_count[p0 + t] = cnt_out;
    a.out_status[p0 + t] = st;
  }
}

// Occupancy: kProteinOcc waves per SIMD (its LDS and VGPR budget); the flat layout's variants
// (a fallback for crowded tables: two full-key mixes per window) need 6 to stay clear of
// scratch.
template <int K, int M, bool Packed>
constexpr int protein_occ() {
  return M == 0 ? 6 : kProteinOcc;
}
template <int K, int M, int P, bool Packed>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(protein_occ<K, M, Packed>(), 8))) void annotate_kernel(
    ProteinArgs a) {
  __shared__ ProteinSmem<P> sm;
  KMA_CLK(0);
  const int t = threadIdx.x;
  // The ASCII kernel's LUT: loaded now, stored to LDS once the first residue loads are issued
  // (its store right here made the block wait for it before loading the offsets: one more
  // dependent round trip per block). Read after annotate_block's first barrier.
  const uint8_t lut_b = Packed ? 0 : a.lut[t];
  // Two-pass grid (defer_below > 0): blocks [0, n_groups) annotate the long groups, blocks
  // [n_groups, 2 n_groups) the short ones, so that every long group starts before any short
  // one (blocks are dispatched in index order); a block whose group is the other pass's exits
  // after reading its offsets.
  const bool second = a.defer_below && blockIdx.x >= a.n_groups;
  GroupHead h;
  WinWords ww[kProbeWin];
  // (the two-pass grid keeps block order: its long-first order is what it is for)
  const uint32_t b = blockIdx.x - (second ? a.n_groups : 0u);
  head_offsets(a, a.defer_below ? b : xcd_group(b, a.n_groups), h);
  if (Packed) {
    head_residues<kProbeWin>(a, h, (uint32_t)t >> 6, chunk_window(t), ww);
  } else {  // the first stage's residue words (clamped to the batch: the span is not known yet)
    uint64_t pos0;
    const uint8_t* res = head_res<false>(a, h, pos0);
    stage_fetch(res, h.steps, 0u, a.n_residues - (uint32_t)h.span_lo, ww);  // (span_lo <= n_residues)
    sm.lut[t] = lut_b;
  }
  annotate_block<K, M, P, Packed>(a, sm, h, ww, a.defer_below ? (second ? 1 : 0) : -1);
  KMA_CLK(5);
  KMA_CLK_HW();
}

// ---------------------------------------------------------------------------------------------
// Residue packing (ASCII -> the packed stream of kma_device.h): a thread turns 64 residues of
// the call (from d_residues + offsets[0]) into 5 stream words (320 bits), codes through the
// table's LUT (0 for a byte without a code). Aligned 8-byte loads around the residues, one
// funnel shift per word; the last, partial group by bytes. Reads 1 B and writes 0.625 B per
// residue: ~0.1 ms for c5's 310M residues.
// ---------------------------------------------------------------------------------------------
// (x[k]: residues 8 k .. 8 k + 7 of the group, byte j = residue j; 40 stream bits each, pack8)
__device__ __forceinline__ void pack64(const uint8_t (&lut)[256], const uint64_t (&x)[8],
                                       uint64_t* __restrict__ out) {
  uint64_t w[5] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t c = pack8(lut, x[i]);
    const int k = (40 * i) >> 6, o = (40 * i) & 63;  // MSB-first bit o of stream word k
    if (o <= 24) {
      w[k] |= c << (24 - o);
    } else {
      w[k] |= c >> (o - 24);
      w[k + 1] |= c << (88 - o);
    }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) out[k] = bswap64(w[k]);  // stream bytes in memory order
}

__global__ __launch_bounds__(256) void pack_residues_kernel(const uint8_t* __restrict__ residues,
                                                            const uint64_t* __restrict__ offsets,
                                                            uint64_t n, const uint8_t* lut_g,
                                                            uint64_t* __restrict__ out) {
  __shared__ uint8_t lut[256];
  lut[threadIdx.x] = lut_g[threadIdx.x];
  __syncthreads();
  const uint8_t* base = residues + offsets[0];
  const uint32_t mis = (uint32_t)((uintptr_t)base & 7u);
  const uint64_t* aligned = reinterpret_cast<const uint64_t*>(base - mis);
  const uint64_t groups = (n + 63) / 64;
  for (uint64_t g = blockIdx.x * 256ull + threadIdx.x; g < groups; g += gridDim.x * 256ull) {
    uint64_t x[8];
    if (64 * g + 64 <= n) {  // whole group: 9 aligned words (the batch is readable past its end)
      uint64_t v[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) v[k] = aligned[8 * g + k];
#pragma unroll
      for (int k = 0; k < 8; ++k) x[k] = funnel(v[k], v[k + 1], mis * 8u);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        x[k] = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint64_t i = 64 * g + 8 * k + j;
          x[k] |= (uint64_t)(i < n ? base[i] : 0u) << (8 * j);
        }
      }
    }
    pack64(lut, x, out + 5 * g);
  }
  if (blockIdx.x == 0 && threadIdx.x < 2) out[5 * groups + threadIdx.x] = 0;  // read padding
}

}  // namespace

// ---- launchers ----------------------------------------------------------------------------------
// The kernel's protein capacity P (its compare chains, protein records and SGPRs scale with
// it): K = 8 kernels come in P = 4 / 6 / 8 and take the smallest that holds the call's block
// proteins (the defaults: 6 at c5, 4 at c2 / c4); other K use P = kBlockProteins.
template <int K, int M, int P>
hipError_t launch_annotate_p(const ProteinArgs& a, dim3 grid, hipStream_t stream) {
  if (a.packed)
    hipLaunchKernelGGL((annotate_kernel<K, M, P, true>), grid, dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL((annotate_kernel<K, M, P, false>), grid, dim3(256), 0, stream, a);
  return hipGetLastError();
}
template <int K, int M>
struct AnnotateLaunch {
  static hipError_t run(const ProteinArgs& a, hipStream_t stream) {
    if constexpr (wide_k(K)) {  // the protein path packs windows of <= 8 residues (one u64)
      return hipErrorInvalidValue;
    } else {
    constexpr int P = kBlockProteins;
    const unsigned bp = a.block_proteins >= 1 && a.block_proteins <= (uint32_t)P ? a.block_proteins : 4u;
    if (bp != a.block_proteins) return hipErrorInvalidValue;
    const unsigned blocks = (a.n_seq + bp - 1) / bp;
    if (a.n_groups != blocks) return hipErrorInvalidValue;
    const dim3 grid(a.defer_below ? 2 * blocks : blocks);
    if constexpr (K == 8 && P > 6) {
      if (bp <= 4) return launch_annotate_p<K, M, 4>(a, grid, stream);
      if (bp <= 6) return launch_annotate_p<K, M, 6>(a, grid, stream);
    }
    return launch_annotate_p<K, M, P>(a, grid, stream);
    }
  }
};

hipError_t launch_annotate(const ProteinArgs& a, hipStream_t stream) {
  if (a.n_seq == 0) return hipSuccess;
  return dispatch_km<AnnotateLaunch>(a.k, a.mlen, a, stream);
}

hipError_t launch_pack_residues(const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                                const uint8_t* lut, uint8_t* out, hipStream_t stream) {
  const uint64_t groups = (n + 63) / 64;
  const unsigned g = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(4096, (groups + 255) / 256));
  hipLaunchKernelGGL(pack_residues_kernel, dim3(g), dim3(256), 0, stream, residues, offsets, n,
                     lut, reinterpret_cast<uint64_t*>(out));
  return hipGetLastError();
}

}  // namespace kma
