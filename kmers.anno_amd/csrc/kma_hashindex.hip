// kma_hashindex.hip — the hash annotator against a resident prototype index (§8(f)3;
// kma_hashindex.h has the index and the pieces shared with the host check program).
//
// HashAnnotationProcessor scores every genome against the same role annotation file
// (HashAnnotationProcessor.java:208, :259-271), so the prototype side (window keys, per-prototype
// sets, set sizes, and here the postings of every distinct key) is built once
// (kma_proto_index_create) and a genome costs only its own side:
//   index_lookup_kernel  every distinct key of the genome's proteins, binary search in the
//                        index's unique keys
//   index_score_kernel   one workgroup per genome protein. Accumulate: the protein's matched keys
//                        in chunks of 256; a chunk's posting lengths are prefix-summed in LDS and
//                        the threads stride the flattened postings (one long posting list is
//                        spread over the block); every prototype id goes into an open-addressed
//                        LDS table (atomicCAS on the ids, atomicAdd on the counts) that persists
//                        across chunks. Score: the table is swept, the similarity of every
//                        entry is the double expression of kma_hash_annotate, entries at or
//                        above min_sim add to out_count, a block reduce keeps the best
//                        (similarity, then the smaller prototype), and the block writes its
//                        protein's out_best / out_sim itself.
// More than CAP distinct prototypes in the table: nothing of the range is published, the range
// is split at its midpoint and both halves are scored in turn (a key's postings ascend, so its
// part of a range is found by lower bound); the running best is carried across ranges. Every
// prototype lies in exactly one scored range and all arithmetic is integer counts and one double
// division, so the results do not depend on CAP or on scheduling.
#include "kma_hashindex.h"
#include "kma_kmersets.h"

namespace kma {
namespace {

__device__ __forceinline__ uint32_t lds_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__global__ __launch_bounds__(256) void index_lookup_kernel(HashIndexArgs a) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < a.n_gpos; i += gridDim.x * 256ull) {
    uint32_t m = kHashEmpty;
    if (a.gfirst[i]) {
      const uint64_t v = a.gsorted[i];
      const uint64_t lo = lower_bound(a.ukeys, 0, a.n_u, v);
      if (lo < a.n_u && a.ukeys[lo] == v) m = (uint32_t)lo;
    }
    a.gmatch[i] = m;
  }
}

// Count one posting. A new prototype claims a free slot only while the distinct count has not
// passed cap (kma_hashindex.h hash_table_slots: a free slot always remains); once it has, the
// range is going to be split and its counts are dropped.
__device__ __forceinline__ void table_add(uint32_t* ids, uint32_t* cnt, uint32_t* distinct,
                                          uint32_t proto, uint32_t bits, uint32_t cap) {
  const uint32_t mask = (1u << bits) - 1u;
  uint32_t h = hash_slot(proto, bits);
  for (uint32_t probe = 0; probe <= mask; ++probe, h = (h + 1) & mask) {
    uint32_t cur = lds_load(ids + h);
    if (cur == kHashEmpty) {
      if (lds_load(distinct) > cap) return;
      cur = atomicCAS(ids + h, kHashEmpty, proto);
      if (cur == kHashEmpty) {
        atomicAdd(distinct, 1u);
        cur = proto;
      }
    }
    if (cur == proto) {
      atomicAdd(cnt + h, 1u);
      return;
    }
  }
  atomicMax(distinct, cap + 1u);  // (a full table: not reached, see above)
}

__global__ __launch_bounds__(256) void index_score_kernel(HashIndexArgs a, uint32_t bits) {
  extern __shared__ uint32_t s_table[];  // ids[T], then counts[T]
  __shared__ uint32_t s_pre[kHashBlock + 1], s_start[kHashBlock], s_wsum[4];
  __shared__ uint32_t s_lo[kHashStackDepth], s_hi[kHashStackDepth], s_n, s_distinct;
  __shared__ uint32_t s_red_lo[4], s_red_hi[4], s_red_id[4];
  const uint32_t T = 1u << bits, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t* ids = s_table;
  uint32_t* cnt = s_table + T;
  const uint64_t o0 = a.goff[0];
  for (uint32_t g = blockIdx.x; g < a.n_genome; g += gridDim.x) {
    const uint64_t seg_lo = a.goff[g] - o0, seg_hi = a.goff[g + 1] - o0;
    const uint32_t gs = a.gsize[g];
    uint64_t best_bits = 0;
    uint32_t best_id = kHashEmpty, ranges = 0;
    bool first = true, has = false, split = false;
    __syncthreads();  // (the protein before: its last reads of the stack and the reduce slots)
    if (tid == 0) {
      HashRangeStack st;
      st.init(s_lo, s_hi, a.n_proto);
      s_n = st.n;
    }
    for (;;) {
      __syncthreads();
      const uint32_t n = s_n;
      if (n == 0) break;
      const uint32_t lo = s_lo[n - 1], hi = s_hi[n - 1];
      __syncthreads();
      if (tid == 0) {
        s_n = n - 1;
        s_distinct = 0;
      }
      for (uint32_t s = tid; s < T; s += kHashBlock) {
        ids[s] = kHashEmpty;
        cnt[s] = 0;
      }
      __syncthreads();
      // ---- accumulate: the protein's keys, a chunk of 256 positions at a time
      for (uint64_t c = seg_lo; c < seg_hi; c += kHashBlock) {
        const uint64_t i = c + tid;
        uint32_t b = 0, len = 0;
        if (i < seg_hi) {
          const uint32_t u = a.gmatch[i];
          if (u != kHashEmpty) {
            uint32_t e = a.pstart[u + 1];
            b = a.pstart[u];
            if (lo) b = postings_lower_bound(a.postings, b, e, lo);
            if (hi < a.n_proto) e = postings_lower_bound(a.postings, b, e, hi);
            len = e - b;
          }
        }
        uint32_t incl = len;  // inclusive scan in the wave, then the waves' sums
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
          const uint32_t up = __shfl_up(incl, d);
          if (lane >= d) incl += up;
        }
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        // (block-uniform: the chunk before has ended, this one's inserts start after the barrier)
        const bool over = lds_load(&s_distinct) > a.cap;
        uint32_t woff = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) {
          const uint32_t v = s_wsum[w];
          woff += w < wave ? v : 0u;
          total += v;
        }
        s_pre[tid] = woff + incl - len;
        s_start[tid] = b;
        if (tid == 0) s_pre[kHashBlock] = total;
        __syncthreads();
        if (over) break;  // the range is going to be split
        for (uint32_t j = tid; j < total; j += kHashBlock) {
          const uint32_t key = prefix_owner(s_pre, kHashBlock, j);
          table_add(ids, cnt, &s_distinct, a.postings[s_start[key] + (j - s_pre[key])], bits,
                    a.cap);
        }
        __syncthreads();
      }
      __syncthreads();
      const uint32_t distinct = lds_load(&s_distinct);
      if (first) has = distinct > 0;
      first = false;
      if (distinct > a.cap) {  // nothing of this range is published
        split = true;
        if (tid == 0) {
          HashRangeStack st{s_lo, s_hi, s_n};
          st.split(lo, hi);
          s_n = st.n;
        }
        continue;
      }
      if (distinct == 0) continue;
      ++ranges;
      // ---- score: sweep the table
      uint64_t my_bits = 0;
      uint32_t my_id = kHashEmpty;
      for (uint32_t s = tid; s < T; s += kHashBlock) {
        const uint32_t id = ids[s];
        if (id == kHashEmpty) continue;
        const double sim = hash_similarity(a.psize[id], gs, cnt[s]);
        if (!(sim >= a.min_sim)) continue;
        atomicAdd(a.out_count + id, 1u);
        const uint64_t sb = (uint64_t)__double_as_longlong(sim);
        if (hash_better(sb, id, my_bits, my_id)) my_bits = sb, my_id = id;
      }
#pragma unroll
      for (uint32_t d = 32; d; d >>= 1) {
        const uint32_t olo = __shfl_xor((uint32_t)my_bits, d);
        const uint32_t ohi = __shfl_xor((uint32_t)(my_bits >> 32), d);
        const uint32_t oid = __shfl_xor(my_id, d);
        const uint64_t ob = (uint64_t)ohi << 32 | olo;
        if (hash_better(ob, oid, my_bits, my_id)) my_bits = ob, my_id = oid;
      }
      if (lane == 0) {
        s_red_lo[wave] = (uint32_t)my_bits;
        s_red_hi[wave] = (uint32_t)(my_bits >> 32);
        s_red_id[wave] = my_id;
      }
      __syncthreads();
#pragma unroll
      for (uint32_t w = 0; w < 4; ++w) {  // every thread: the range's best into the running best
        const uint64_t rb = (uint64_t)s_red_hi[w] << 32 | s_red_lo[w];
        const uint32_t rid = s_red_id[w];
        if (hash_better(rb, rid, best_bits, best_id)) best_bits = rb, best_id = rid;
      }
    }
    if (tid == 0) {
      const bool none = best_id == kHashEmpty;
      a.out_best[g] = none ? -1 : (int32_t)best_id;
      a.out_sim[g] = none ? 0.0 : __longlong_as_double((long long)best_bits);
      if (has) atomicAdd(a.stats, 1ull);
      if (split) atomicAdd(a.stats + 1, 1ull);
      if (ranges) atomicAdd(a.stats + 2, (unsigned long long)ranges);
    }
  }
}

}  // namespace

hipError_t launch_index_lookup(const HashIndexArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(index_lookup_kernel, dim3(grid1(a.n_gpos)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_index_score(const HashIndexArgs& a, hipStream_t s) {
  if (a.cap < 1 || a.cap > kHashCapMax || a.n_genome == 0) return hipErrorInvalidValue;
  const uint32_t slots = hash_table_slots(a.cap);
  const unsigned grid = a.n_genome > (1u << 20) ? (1u << 20) : a.n_genome;
  hipLaunchKernelGGL(index_score_kernel, dim3(grid), dim3(kHashBlock), slots * 8u, s, a,
                     hash_log2(slots));
  return hipGetLastError();
}

}  // namespace kma
