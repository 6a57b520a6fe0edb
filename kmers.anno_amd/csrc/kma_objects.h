// kma_objects.h — the objects behind the C ABI's opaque handles (kma_workspace, kma_table,
// kma_proto_index), a table's replicas and host-context pool, and the phase clock of timed device calls. Shared by
// the kma_abi_*.cpp units; private to the library, not installed.
#pragma once
#include "kma_host.h"
#include "kma_shard_plan.h"

// ---- objects ---------------------------------------------------------------------------------
struct kma_workspace {
  int device = 0;
  int n_cu = 256;
  uint32_t* d_gset = nullptr;  // protein sets that do not fit in LDS: 2 u32 per residue
  uint8_t* d_packed = nullptr; // the call's residues packed (kma_internal.h packed_bytes)
  bool host_ctx = false;       // a host context's workspace: no d_packed (kma_annotate_proteins)
  uint64_t res_cap = 0;        // residues per call
  // 6-frame path (kma_workspace_reserve_contigs): staged hits, block counts, scan.
  kma_hit* d_cstage = nullptr;
  uint32_t* d_ccounts = nullptr;
  // Emit-offset group sums (cgroups u64) and the emit pass's done counter (one u64 after
  // them): zero between calls — the probe adds into the sums, the emit pass's last block
  // zeroes both — so a call keeps no host state and may be graph-captured.
  uint64_t* d_cprefix = nullptr;
  uint64_t cgroups = 0;
  bool cpending = false;  // a probe was set up whose emit pass has not been enqueued
  uint64_t contig_cap = 0;  // bases
  // Per-workspace overrides of KMA_OPT_BLOCK_PROTEINS / KMA_OPT_DEFER (kOptUnset: the default).
  int64_t opt_block_proteins = kma::host::kOptUnset;
  int64_t opt_defer = kma::host::kOptUnset;
  // Per-phase timing (kma_workspace_timing): a ring of calls, each kMaxEv events (phase i runs
  // from event i to event i + 1) and its phase names.
  bool timing = false;
  std::vector<hipEvent_t> events;
  std::vector<const char* const*> names;  // per ring slot
  std::vector<int> n_phases;              // per ring slot
  uint32_t n_timed = 0;
};

namespace kma {
namespace host {
constexpr uint32_t kTimingRing = 256;  // timed calls a workspace remembers
constexpr int kMaxEv = 8;  // events per timed call

// One replica of a table's slot array on one device.
struct Replica {
  int device = 0;
  uint64_t* d_slots = nullptr;
  bool owned = false;
  uint8_t* d_lut = nullptr;
};

// Per-call resources of the host entry points on one device (kept in the table's pool); a
// protein call uses one set of events per piece (kMaxPieces, kma_shard_plan.h).
struct HostCtx {
  int device = 0;
  hipStream_t stream = nullptr;
  // H2D of piece i + 1 under the kernel of piece i, pieces alternating over two copy streams
  // (two DMA engines: 57 vs 50 GB/s for c5's packed stream, profiles/r04/link_r04g.json)
  hipStream_t copy[2] = {};
  hipStream_t d2h = nullptr;  // pieces' outputs back while later pieces copy and run
  hipEvent_t piece_ready[kMaxPieces] = {};
  hipEvent_t piece_ready2[kMaxPieces] = {};  // streamed copies: piece i's data on copy[1]
  hipEvent_t piece_done[kMaxPieces] = {};  // piece i's kernel (on `stream`)
  hipEvent_t out_ready[kMaxPieces] = {};   // piece i's outputs in pinned memory (on d2h)
  kma_workspace* ws = nullptr;
  Grow<uint8_t> d_in;     // residues / DNA (+ padding)
  Grow<uint64_t> d_off;   // offsets
  Grow<uint8_t> d_out;    // outputs (fid, count, tally, status / hit count, tally)
  Grow<uint32_t> d_aux;   // 6-frame STRICT: locations per table slot
  Grow<kma_hit> d_hits;   // 6-frame hits
  Pinned h_in, h_out;     // pinned staging for both directions
};
}  // namespace host
}  // namespace kma

struct kma_table {
  int k = 8;
  int mlen = 6;  // layout: minimizer length, 0 = flat
  bool two_choice = false;  // placement (kma_internal.h alt_bucket): else overflow chains
  uint64_t n_buckets = 0;
  uint8_t lut[256] = {};
  kma_table_info info = {};
  // Replicas: appended by kma_table_replicate while host or device calls may run on the table,
  // so they are read and appended under reps_mu; calls work on a copy (replicas() below).
  std::vector<kma::host::Replica> reps;
  mutable std::mutex reps_mu;
  std::mutex pool_mu;
  std::vector<kma::host::HostCtx*> idle;  // host contexts not in use
};

// The hash annotator's resident prototype index (kma_hashindex.h): read-only after
// kma_proto_index_create, so calls may share it across threads; each call owns its scratch.
struct kma_proto_index {
  int device = 0;
  int k = 8;
  uint32_t n_proto = 0;
  uint64_t n_keys = 0, n_postings = 0, bytes = 0;
  uint64_t* d_keys = nullptr;      // n_keys sorted unique window keys
  uint32_t* d_start = nullptr;     // n_keys + 1 posting starts
  uint32_t* d_postings = nullptr;  // n_postings prototypes, ascending per key
  uint32_t* d_psize = nullptr;     // distinct kmers per prototype
  kma_proto_index() = default;
  kma_proto_index(const kma_proto_index&) = delete;
  kma_proto_index& operator=(const kma_proto_index&) = delete;
  ~kma_proto_index() {
    for (void* q : {(void*)d_keys, (void*)d_start, (void*)d_postings, (void*)d_psize})
      if (q) (void)hipFree(q);
  }
};

// The streamed signature build (kma_sigmerge.h): the resident run of unique ascending keys with
// their states in run_*[cur], the merge target in run_*[cur ^ 1] (swapped in when an add has
// succeeded), and the batch scratch, kept at the largest size seen. Used by one thread at a time.
struct kma_sig_builder {
  int device = 0;
  int k = 8;
  uint32_t flags = 0;
  uint32_t n_adds = 0;
  uint64_t n_residues = 0;
  uint64_t n_keys = 0;        // rows of the resident run
  uint64_t counts[3] = {};    // of them: role / conflict / buffered
  int cur = 0;
  kma::host::Grow<uint64_t> run_keys[2];
  kma::host::Grow<uint32_t> run_states[2];
  // batch scratch: the staged batch, the (key, tag) pairs before and after the sort (the reduced
  // batch lands in ka / ta), head indices then states, run ids, head flags, the merge's tile
  // counts and offsets, the sort / scan / select scratch
  kma::host::Grow<uint8_t> in;
  kma::host::Grow<uint64_t> off;
  kma::host::Grow<int32_t> roles;
  kma::host::Grow<uint64_t> ka, kb;
  kma::host::Grow<uint32_t> ta, tb, head, run;
  kma::host::Grow<uint8_t> hflags;
  kma::host::Grow<uint64_t> tiles;
  kma::host::Grow<uint8_t> temp;
  uint8_t* d_small = nullptr;  // the LUT (256 B), then alpha flag, reduced count, state counts
  // the last merging add's stages (kma_debug_sig_builder_ms): events around windows, sort,
  // reduce, the merge's count pass with its scan, its write pass, the counts
  hipEvent_t ev[9] = {};
  double stage_ms[6] = {};
  kma_sig_builder() = default;
  kma_sig_builder(const kma_sig_builder&) = delete;
  kma_sig_builder& operator=(const kma_sig_builder&) = delete;
  ~kma_sig_builder() {
    for (auto& g : run_keys) g.release();
    for (auto& g : run_states) g.release();
    in.release(), off.release(), roles.release(), ka.release(), kb.release(), ta.release();
    tb.release(), head.release(), run.release(), hflags.release(), tiles.release();
    temp.release();
    if (d_small) (void)hipFree(d_small);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace kma {
namespace host {
// ---- tables (kma_abi_table.cpp) -----------------------------------------------------------------
// Take a host context for `device` from the table's pool (or make one); give it back.
int acquire_ctx(kma_table* t, int device, HostCtx** out);
void release_ctx(kma_table* t, HostCtx* c);
struct CtxGuard {
  kma_table* t;
  HostCtx* c;
  ~CtxGuard() {
    if (!c) return;
    // A call that failed after queueing work returns early: let the context's copies and
    // kernels drain before the next call reuses its pinned and device buffers.
    for (hipStream_t cs : c->copy) (void)hipStreamSynchronize(cs);
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->d2h);
    release_ctx(t, c);
  }
};
// A copy of the table's replicas (safe against a concurrent kma_table_replicate); the one on
// `device`, if any.
std::vector<Replica> replicas(const kma_table* t);
bool replica_on(const kma_table* t, int device, Replica* out);
// Table from device-resident keys / fids on `device` (kma_peg_table_create builds its own keys).
int create_from_device_keys(const uint64_t* d_keys, const uint32_t* d_fids, uint64_t n, int k,
                            int device, double lf, const uint8_t lut[256], kma_table** out);

// ---- workspaces ---------------------------------------------------------------------------------
void free_contig_scratch(kma_workspace* ws);  // kma_abi_contigs.cpp
// The 6-frame device call's phase names (kma_abi_contigs.cpp); kma_workspace_timing_read tells
// a contig call by their address.
extern const char* const kContigPhases[2];

// Records the phase boundaries of one timed device call (nothing when timing is off).
struct PhaseClock {
  hipEvent_t* ev = nullptr;
  int n = 0;
  hipStream_t s = nullptr;
  PhaseClock(kma_workspace* ws, hipStream_t stream, const char* const* names, int n_phases)
      : s(stream) {
    if (!ws->timing) return;
    const uint32_t slot = ws->n_timed++ % kTimingRing;
    ev = &ws->events[kMaxEv * slot];
    ws->names[slot] = names;
    ws->n_phases[slot] = n_phases;
  }
  hipError_t mark() { return ev ? hipEventRecord(ev[n++], s) : hipSuccess; }
};

}  // namespace host
}  // namespace kma
