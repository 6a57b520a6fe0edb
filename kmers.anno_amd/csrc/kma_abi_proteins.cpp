// kma_abi_proteins.cpp — the workspace entry points and the protein path of the C ABI
// (include/kmeranno.h): the device entry points, the host pipeline (protein_shard) and the
// residue packer.
//
// Host entry points (kma_annotate_proteins / kma_annotate_contigs) reuse per-table host
// contexts — a stream, a workspace, device buffers and pinned staging buffers per device —
// taken from the table's pool for the duration of one call, so a per-genome caller pays no
// allocation and concurrent callers never synchronise each other (each waits on its own
// stream only). A table may be replicated on several devices; a host call then cuts its batch
// into residue-balanced contiguous shards, one host thread per replica.
#include <chrono>
#include <memory>

#include "kma_internal.h"
#include "kma_objects.h"
#include "kma_pack.h"

using namespace kma::host;

namespace {
// MI355X's Infinity Cache (MALL): tables larger than this are probed from HBM.
constexpr uint64_t kInfinityCacheBytes = 256ull << 20;

constexpr uint64_t kResPad = 64;            // workspace positions past the last residue
constexpr uint64_t kMaxResidues = (1ull << 32) - 2 * kResPad;  // positions are u32 in kernels

void free_protein_scratch(kma_workspace* ws) {
  if (ws->d_gset) (void)hipFree(ws->d_gset);
  if (ws->d_packed) (void)hipFree(ws->d_packed);
  ws->d_gset = nullptr;
  ws->d_packed = nullptr;
  ws->res_cap = 0;
}

const char* const kDirectPhases[] = {"annotate_kernel"};
const char* const kPackedPhases[] = {"pack_kernel", "annotate_kernel"};

// Proteins per annotate_kernel block (KMA_BLOCK_PROTEINS=1..8 overrides, read per call): 6 for
// batches of more than 4 resident waves of such blocks against a table larger than the Infinity
// Cache, else 4. A block's fixed costs (the
// offsets and first residues round trips, the final chain walks, the vote) are amortized over
// more probe steps with more proteins, while a batch of few waves of blocks ends with a longer
// tail. Measured on MI355X (profiles/r03_ab/r03m, r03n): c5 3.94 / 3.77 / 3.88 ms at 4 / 6 / 8
// (3.87 / 3.72 / 3.84 with queued keys), c2 51 vs 66 us at 4 vs 6. (Round 2, before the walk
// queue and the scratch fix: c5 4.53 / 4.66 / 4.86 ms at 4 / 6 / 8, r02f_block_proteins.log.)
// Round 3 (interleaved A/B, profiles/r03_session2/r03bp_steps.log): c5 (10^8 rows, 1.5 GiB
// table in HBM) 3.59-3.63 / 3.69-3.71 / 3.80-3.81 ms at 6 / 7 / 8; c4 (10^7 rows, a 153 MiB
// table inside the 256 MiB Infinity Cache) 2.752 vs 2.819 ms at 4 vs 6: 6 only for tables
// larger than the Infinity Cache. Round 5, c2 (profiles/r05/c2_opts_r05t/, two runs each):
// 46.6 us at 4 proteins (two-pass grid), 52.4 / 50.0 / 48.0 / 53.9 / 56.6 us at 2 / 3 / 5 / 6 / 8,
// 52.8 without the two-pass grid; and a tapered tail (the batch's last groups of half size, then
// single proteins, so the last blocks to start end sooner; profiles/r05/c2_taper_r05u/) 47.0 /
// 49.3 / 54.0 / 55.1 us for tails of 1/4, 1/2, 1 and 2 resident waves: each group's fixed chain
// (offsets, first residues, final walks, vote) costs more than the shorter tail saves.
uint32_t block_proteins(const kma_workspace* ws, uint32_t n_seq, uint64_t table_bytes) {
  const int64_t f = ws->opt_block_proteins != kOptUnset ? ws->opt_block_proteins
                                                         : opt(KMA_OPT_BLOCK_PROTEINS);
  if (f >= 1 && f <= kma::kBlockProteins) return (uint32_t)f;
  const uint64_t slots = (uint64_t)kma::kProteinOcc * (uint64_t)std::max(ws->n_cu, 1);
  return (uint64_t)n_seq / 6 > 4 * slots && table_bytes > kInfinityCacheBytes ? 6u : 4u;
}

// Deferral of short groups (annotate_kernel's two-pass grid), in probe steps: groups below it
// are annotated after every longer one has started. A fixed-count grid is dispatched in
// block order, so without it a long group dispatched late ends the call alone: at c2 the
// kernel's last ~25 of ~65 us ran with a shrinking set of late long blocks
// (profiles/r02m_block_clock.jsonl; with the groups pre-sorted longest first the kernel took
// 50 us). Automatic for grids of more than one and at most 4 resident waves of blocks (7 per
// CU): measured (profiles/r02m_defer_ab.log) c2 (1.4 waves) 66 -> 54 us, 40k proteins (5.6)
// even, 100k (14) 3% slower, c4 / c5 7% / 3% slower when forced. KMA_DEFER=0 disables it,
// KMA_DEFER=<steps> forces it on any batch (read per call).
uint32_t defer_below(const kma_workspace* ws, uint64_t n_groups) {
  const uint64_t slots = (uint64_t)kma::kProteinOcc * (uint64_t)std::max(ws->n_cu, 1);
  const int64_t f = ws->opt_defer != kOptUnset ? ws->opt_defer : opt(KMA_OPT_DEFER);
  if (f >= 0) return (uint32_t)std::min<int64_t>(64, f);
  return n_groups > slots && n_groups <= 4 * slots ? 3u : 0u;
}

// How the protein kernel gets its residues: ASCII, which each block packs into its LDS stage
// as it goes (the device entry point's default); ASCII packed on the device first (pack_kernel
// into the workspace, then the packed kernel: KMA_OPT_PACKED_INPUT = 2); a packed stream the
// caller staged (host entry, packed device entry; stream residue `stream_first` = residue
// offsets[0]).
enum class Input { kAscii, kPackOnDevice, kStream };

// Device calls of every size run the staged ASCII probe alone under KMA_OPT_PACKED_INPUT = 0 and
// 1 (the default): the pack pass read 1 B and wrote 0.625 B per residue for the probe to read
// back, a launch and ~0.1 ms of c5's step on the fabric the probe is bound by.
// 2 keeps the pack kernel + stream probe: the control arm of that measurement. Host calls pack
// under 1 and 2 (the H2D is the bound there).
bool pack_on_device(uint64_t n_residues) {
  return n_residues > 0 && opt(KMA_OPT_PACKED_INPUT) == 2;
}

// The workspace's packed stream for device calls that pack: allocated by
// kma_workspace_reserve_batch (never here: the device entry points do not allocate).
int ensure_packed(const kma_workspace* ws) {
  if (ws->d_packed) return KMA_OK;
  return fail(KMA_E_CAPACITY, "workspace has no packed stream (kma_workspace_reserve_batch first)");
}

// The protein path on one replica (device buffers, asynchronous on s).
int annotate_proteins_on(const kma_table* t, const Replica& r, kma_workspace* ws,
                         const uint8_t* d_residues, const uint64_t* d_offsets, uint32_t n_seq,
                         uint64_t n_residues, int min_hits, uint32_t flags, int32_t* d_fid,
                         int32_t* d_count, uint8_t* d_status, uint32_t* d_tally, uint32_t n_fid,
                         hipStream_t s, Input input = Input::kAscii, uint64_t stream_first = 0) {
  kma::ProteinArgs a{};
  a.slots = r.d_slots;
  a.n_buckets = (uint32_t)t->n_buckets;
  a.lut = r.d_lut;
  a.residues = input == Input::kPackOnDevice ? ws->d_packed : d_residues;
  a.packed = input != Input::kAscii;
  a.stream_first = input == Input::kStream ? stream_first : 0;
  a.offsets = d_offsets;
  a.n_seq = n_seq;
  a.n_residues = (uint32_t)n_residues;
  a.k = t->k;
  a.mlen = t->mlen;
  a.two_choice = t->two_choice ? 1u : 0u;
  a.min_hits = min_hits;
  a.flags = flags;
  a.out_fid = d_fid;
  a.out_count = d_count;
  a.out_status = d_status;
  a.tally = d_tally;
  a.n_fid = d_tally ? n_fid : 0;
  a.gset = ws->d_gset;
  a.block_proteins = block_proteins(ws, n_seq, t->n_buckets * (uint64_t)kma::kBucketBytes);
  a.n_groups = (n_seq + a.block_proteins - 1) / a.block_proteins;
  a.defer_below = a.n_groups < (1u << 30) ? defer_below(ws, a.n_groups) : 0u;
  const bool pack = input == Input::kPackOnDevice;
  PhaseClock clk(ws, s, pack ? kPackedPhases : kDirectPhases, pack ? 2 : 1);
  KMA_HIP(clk.mark());
  if (pack) {
    KMA_HIP(kma::launch_pack_residues(d_residues, d_offsets, n_residues, r.d_lut, ws->d_packed,
                                      s));
    KMA_HIP(clk.mark());
  }
  KMA_HIP(kma::launch_annotate(a, s));
  KMA_HIP(clk.mark());
  return KMA_OK;
}

int check_protein_call(const kma_table* t, int min_hits, uint32_t flags) {
  if (!t) return fail(KMA_E_INVALID, "null table");
  if (kma::wide_k(t->k))
    return fail(KMA_E_INVALID, "the protein path takes tables of K <= 8 (this table: K = %d)",
                t->k);
  if (min_hits < 1) return fail(KMA_E_INVALID, "Min-hits must be positive.");
  if (flags & ~(KMA_F_END_EXCLUSIVE | KMA_F_MULTISET)) return fail(KMA_E_INVALID, "bad flags");
  return KMA_OK;
}

// The argument checks of the device entry points; d_in is the residues or the packed stream
// (`what` in the alignment message). *out: the table's replica on the workspace's device. A call
// of no proteins passes without its buffers being looked at (the caller returns then).
int check_device_call(const kma_table* t, const kma_workspace* ws, const uint8_t* d_in,
                      const char* what, const uint64_t* d_offsets, uint32_t n_seq,
                      uint64_t n_residues, int min_hits, uint32_t flags, const int32_t* d_fid,
                      const int32_t* d_count, const uint8_t* d_status, Replica* out) {
  if (int rc = check_protein_call(t, min_hits, flags)) return rc;
  if (!ws) return fail(KMA_E_INVALID, "null workspace");
  if (!replica_on(t, ws->device, out))
    return fail(KMA_E_INVALID, "table has no replica on the workspace's device %d", ws->device);
  if (n_seq == 0) return KMA_OK;
  if (!d_in || !d_offsets || !d_fid || !d_count || !d_status)
    return fail(KMA_E_INVALID, "null device buffer");
  if ((uintptr_t)d_in & 7) return fail(KMA_E_INVALID, "%s must be 8-byte aligned", what);
  if (n_residues > kMaxResidues)
    return fail(KMA_E_INVALID, "%llu residues in one call (limit 2^32 - 128)",
                (unsigned long long)n_residues);
  if (n_residues > ws->res_cap)
    return fail(KMA_E_CAPACITY, "workspace reserved for %llu residues, call needs %llu",
                (unsigned long long)ws->res_cap, (unsigned long long)n_residues);
  return KMA_OK;
}
}  // namespace

// Host bytes -> pinned staging -> device: the staging pool copies the bytes into the pinned
// buffer in 2 MiB chunks and ONE copy goes on s (r04g's trace of 153 chunk-sized copies kept the
// DMA engine idle a quarter of the time, profiles/r04/e2e_trace_r04g.json).
hipError_t kma::host::stage_h2d(uint8_t* d_dst, uint8_t* h_pinned, const uint8_t* src, size_t len,
                                hipStream_t s) {
  constexpr size_t kChunk = 2u << 20;
  const size_t n_chunks = (len + kChunk - 1) / kChunk;
  staging_pool().run(n_chunks, staging_threads(), [&](uint64_t i) {
    const size_t off = i * kChunk;
    std::memcpy(h_pinned + off, src + off, std::min(kChunk, len - off));
  });
  return len ? hipMemcpyAsync(d_dst, h_pinned, len, hipMemcpyHostToDevice, s) : hipSuccess;
}

namespace {
// Host-side phase times of the last host protein shard call (kma_debug_host_profile, for the
// host-call measurements in scripts/e2e_host.py): ms in setup (context, reservations, offsets),
// staging (packing / copying into pinned memory and queueing the copies), launches, the final
// wait for the stream, the output copies, and the whole call; then the staging width and the
// pieces. Also per replica (the first kProfReplicas of a fanned-out call).
constexpr int kProfFields = 8, kProfReplicas = 64;
std::mutex g_prof_mu;
double g_prof[kProfFields] = {};
double g_prof_rep[kProfReplicas][kProfFields] = {};
using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point a) {
  return std::chrono::duration<double, std::milli>(Clock::now() - a).count();
}

// One shard of a host protein call on one replica, while the call runs. Host bytes -> pinned
// staging -> device, pipelined: the shard is cut into pieces of whole proteins (plan), one kernel
// per piece on the compute stream s, behind the piece's input on the copy streams; a piece's
// outputs go back on the d2h stream while later pieces copy and run. The call's inputs are fixed
// at construction; bind() takes the pointers into the context's buffers once protein_shard has
// reserved them, then protein_shard sets the plan.
struct Shard {
  kma_table* const t;
  const Replica& r;
  HostCtx* const c;
  const hipStream_t s;  // c->stream
  const ShardLayout lay;
  const uint8_t* const residues;  // the shard's first residue in the caller's array
  const uint64_t nres, n_groups;  // n_groups: stream groups of 64 residues
  const bool packed;
  const size_t in_bytes;  // the staged input with the kernel's read padding
  const int min_hits;
  const uint32_t flags;
  uint8_t* hin = nullptr;          // pinned: the staged input, then the offsets
  const uint64_t* hoff = nullptr;  // the shard's offsets rebased to 0
  int32_t* d_fid = nullptr;
  int32_t* d_cnt = nullptr;
  uint32_t* d_tally = nullptr;
  uint8_t* d_st = nullptr;
  PiecePlan plan;
  double t_stage = 0, t_launch = 0, t_wait = 0;  // ms (the profile)

  Shard(kma_table* t, const Replica& r, HostCtx* c, ShardLayout lay, const uint8_t* residues,
        uint64_t nres, bool packed, int min_hits, uint32_t flags)
      : t(t), r(r), c(c), s(c->stream), lay(lay), residues(residues), nres(nres),
        n_groups((nres + 63) / 64), packed(packed),
        in_bytes(packed ? (size_t)kma::packed_bytes(nres) : (nres + kResPad + 7) & ~7ull),
        min_hits(min_hits), flags(flags) {}
  uint64_t* bind();
  int outputs_back(int i, uint32_t a, uint32_t b);
  int launch_piece(int i, hipStream_t cs, bool both_copies = false);
  int stage_streamed();
  int stage_piecewise();
  int collect_outputs(int32_t* out_fid, int32_t* out_count, uint8_t* out_status, uint32_t* tally);
};

// The pointers into the context's reserved buffers; returns the pinned offsets array (n + 1
// entries behind the staged input) for the caller to fill.
uint64_t* Shard::bind() {
  hin = c->h_in.p;
  uint64_t* off = reinterpret_cast<uint64_t*>(hin + in_bytes);
  hoff = off;
  uint8_t* dout = c->d_out.p;
  d_fid = reinterpret_cast<int32_t*>(dout + lay.fid_at);
  d_cnt = reinterpret_cast<int32_t*>(dout + lay.count_at);
  d_tally = lay.tally ? reinterpret_cast<uint32_t*>(dout + lay.tally_at) : nullptr;
  d_st = dout + lay.status_at;
  return off;
}

// Piece i's outputs back on the d2h stream once its kernel is done (fid, count, status slices;
// the tally with the last piece), while later pieces copy and run.
int Shard::outputs_back(int i, uint32_t a, uint32_t b) {
  KMA_HIP(hipEventRecord(c->piece_done[i], s));
  KMA_HIP(hipStreamWaitEvent(c->d2h, c->piece_done[i], 0));
  uint8_t* h = c->h_out.p;
  if (b > a) {
    KMA_HIP(hipMemcpyAsync(h + lay.fid_at + a * 4ull, d_fid + a, (b - a) * 4ull,
                           hipMemcpyDeviceToHost, c->d2h));
    KMA_HIP(hipMemcpyAsync(h + lay.count_at + a * 4ull, d_cnt + a, (b - a) * 4ull,
                           hipMemcpyDeviceToHost, c->d2h));
    KMA_HIP(hipMemcpyAsync(h + lay.status_at + a, d_st + a, b - a, hipMemcpyDeviceToHost, c->d2h));
  }
  if (i + 1 == plan.n_pieces && lay.tally)
    KMA_HIP(hipMemcpyAsync(h + lay.tally_at, d_tally, lay.n_fid * 4ull, hipMemcpyDeviceToHost,
                           c->d2h));
  KMA_HIP(hipEventRecord(c->out_ready[i], c->d2h));
  return KMA_OK;
}

// Piece i's kernel (after its input is on the device: piece_ready[i] on copy stream cs, and
// with both_copies, piece_ready2[i] on copy[1] as well) and the copy of its outputs.
int Shard::launch_piece(int i, hipStream_t cs, bool both_copies) {
  const uint32_t a = plan.pbeg[i], b = plan.pbeg[i + 1];
  KMA_HIP(hipEventRecord(c->piece_ready[i], cs));
  KMA_HIP(hipStreamWaitEvent(s, c->piece_ready[i], 0));
  if (both_copies) {
    KMA_HIP(hipEventRecord(c->piece_ready2[i], c->copy[1]));
    KMA_HIP(hipStreamWaitEvent(s, c->piece_ready2[i], 0));
  }
  if (b > a)
    if (int rc = annotate_proteins_on(t, r, c->ws, c->d_in.p, c->d_off.p + a, b - a,
                                      hoff[b] - hoff[a], min_hits, flags, d_fid + a, d_cnt + a,
                                      d_st + a, d_tally, lay.n_fid, s,
                                      packed ? Input::kStream : Input::kAscii, hoff[a]))
      return rc;
  return outputs_back(i, a, b);
}

// Packed input: the whole stream is packed by ONE staging-pool job in chunks, in stream order,
// and the calling thread copies it in segments (plan_segments: never across a piece boundary) as
// soon as a segment's chunks are all packed, packing chunks itself while it waits; a piece's
// kernel follows its last segment. (Packing a whole piece before its one copy left the link
// idle while each piece was packed: DESIGN 5, "The host call".)
int Shard::stage_streamed() {
  const SegShape shape;
  const SegPlan sp = plan_segments(plan, hoff, n_groups, shape);
  const std::vector<Seg>& segs = sp.segs;
  const uint64_t tail = in_bytes - 40 * n_groups;  // the kernel's read padding, zeroed
  std::unique_ptr<std::atomic<uint32_t>[]> left(new std::atomic<uint32_t>[segs.size()]);
  for (size_t k = 0; k < segs.size(); ++k) left[k].store(segs[k].chunks, std::memory_order_relaxed);
  int rc_copy = KMA_OK;
  staging_pool().run_with(
      sp.chunk_seg.size(), staging_threads(),
      [&](uint64_t ci) {
        const Seg& sg = segs[sp.chunk_seg[ci]];
        const uint64_t g0 = sp.chunk_g0[ci], g1 = std::min(sg.g1, g0 + shape.chunk_groups);
        const uint64_t r0 = 64 * g0, r1 = std::min(64 * g1, nres);
        const uint64_t bytes = 40 * (g1 - g0) + (g1 == n_groups ? tail : 0);
        kma::pack_residues_host(t->lut, residues + r0, r1 > r0 ? r1 - r0 : 0, hin + 40 * g0,
                                bytes);
        left[sp.chunk_seg[ci]].fetch_sub(1, std::memory_order_release);
      },
      [&](auto& help) {
        for (size_t k = 0; k < segs.size() && rc_copy == KMA_OK; ++k) {
          const Clock::time_point t_w = Clock::now();
          while (left[k].load(std::memory_order_acquire) != 0)
            if (!help()) std::this_thread::yield();
          const Clock::time_point t_issue = Clock::now();
          t_stage += std::chrono::duration<double, std::milli>(t_issue - t_w).count();
          const Seg& sg = segs[k];
          // Segments alternate over the two copy streams (two DMA engines: 52 vs 44 GB/s on
          // one stream, profiles/r05/e2e_streamed_fifo_r05i), in stream order on each, and a
          // piece's kernel waits for both: a piece's data lands as early as the link allows.
          hipStream_t cs = c->copy[0];
          if (k & 1) cs = c->copy[1];
          const uint64_t bytes = 40 * (sg.g1 - sg.g0) + (sg.g1 == n_groups ? tail : 0);
          if (sg.g1 == n_groups && sg.chunks == 0) std::memset(hin + 40 * n_groups, 0, tail);
          if (bytes) {
            const hipError_t e = hipMemcpyAsync(c->d_in.p + 40 * sg.g0, hin + 40 * sg.g0, bytes,
                                                hipMemcpyHostToDevice, cs);
            if (e != hipSuccess)
              rc_copy = fail(KMA_E_DEVICE, "hipMemcpyAsync: %s", hipGetErrorString(e));
          }
          if (rc_copy == KMA_OK && sg.last) rc_copy = launch_piece(sg.piece, c->copy[0], true);
          t_launch += ms_since(t_issue);
        }
        while (help()) {}  // (after an error: the job still completes)
      });
  return rc_copy;
}

// ASCII input: the staging pool copies piece i's part into the pinned buffer and ONE copy per
// piece (stage_h2d) goes on copy stream i % 2, so piece i + 1 is staged while piece i's copy and
// kernel run; the zero padding follows the last piece.
int Shard::stage_piecewise() {
  for (int i = 0; i < plan.n_pieces; ++i) {
    hipStream_t cs = c->copy[i & 1];
    const Clock::time_point t_piece = Clock::now();
    const uint64_t ra = hoff[plan.pbeg[i]];
    const uint64_t rb = i + 1 < plan.n_pieces ? hoff[plan.pbeg[i + 1]] : nres;
    KMA_HIP(stage_h2d(c->d_in.p + ra, hin + ra, residues + ra, rb - ra, cs));
    if (i + 1 == plan.n_pieces) {
      std::memset(hin + nres, 0, in_bytes - nres);
      KMA_HIP(hipMemcpyAsync(c->d_in.p + nres, hin + nres, in_bytes - nres, hipMemcpyHostToDevice,
                             cs));
    }
    const Clock::time_point t_staged = Clock::now();
    t_stage += std::chrono::duration<double, std::milli>(t_staged - t_piece).count();
    if (int rc = launch_piece(i, cs)) return rc;
    t_launch += ms_since(t_staged);
  }
  return KMA_OK;
}

// Pieces' outputs into the caller's arrays (of the shard's first protein onwards) as they
// arrive: the later pieces still copy and run meanwhile.
int Shard::collect_outputs(int32_t* out_fid, int32_t* out_count, uint8_t* out_status,
                           uint32_t* tally) {
  const uint8_t* h = c->h_out.p;
  for (int i = 0; i < plan.n_pieces; ++i) {
    const Clock::time_point t_w = Clock::now();
    KMA_HIP(hipEventSynchronize(c->out_ready[i]));
    t_wait += ms_since(t_w);
    const uint32_t a = plan.pbeg[i], b = plan.pbeg[i + 1];
    if (b == a) continue;
    pool_memcpy(out_fid + a, h + lay.fid_at + a * 4ull, (b - a) * 4ull);
    pool_memcpy(out_count + a, h + lay.count_at + a * 4ull, (b - a) * 4ull);
    pool_memcpy(out_status + a, h + lay.status_at + a, b - a);
  }
  if (lay.tally) std::memcpy(tally, h + lay.tally_at, lay.n_fid * 4ull);
  return KMA_OK;
}

// One shard [lo, hi) of a host protein call on replica r (host buffers, synchronous).
int protein_shard(kma_table* t, const Replica& r, int rep, const uint8_t* residues,
                  const uint64_t* offsets, uint32_t lo, uint32_t hi, int min_hits,
                  uint32_t flags, int32_t* out_fid, int32_t* out_count, uint8_t* out_status,
                  uint32_t* tally, uint32_t n_fid) {
  const uint32_t n = hi - lo;
  if (n == 0) return KMA_OK;
  const Clock::time_point t_call = Clock::now();
  const uint64_t base = offsets[lo], nres = offsets[hi] - base;
  if (nres > kMaxResidues)
    return fail(KMA_E_INVALID, "a protein of %llu residues (limit 2^32 - 128)",
                (unsigned long long)nres);
  HostCtx* c = nullptr;
  if (int rc = acquire_ctx(t, r.device, &c)) return rc;
  CtxGuard guard{t, c};
  DeviceScope ds(r.device);
  if (ds.err != hipSuccess) return fail(KMA_E_DEVICE, "hipSetDevice(%d)", r.device);
  // KMA_OPT_PACKED_INPUT (default): residues are packed to 5 bits while they are staged (the
  // H2D moves 0.625 bytes per residue) and the packed kernel reads the stream.
  Shard sh(t, r, c, ShardLayout(n, n_fid, tally != nullptr), residues + base, nres,
           opt(KMA_OPT_PACKED_INPUT) != 0, min_hits, flags);
  const size_t off_bytes = (n + 1) * 8ull;
  KMA_HIP(c->d_in.reserve(sh.in_bytes));
  KMA_HIP(c->d_off.reserve(n + 1));
  KMA_HIP(c->d_out.reserve(sh.lay.out_bytes));
  KMA_HIP(c->h_in.reserve(sh.in_bytes + off_bytes));
  KMA_HIP(c->h_out.reserve(sh.lay.out_bytes));
  if (int rc = kma_workspace_reserve_batch(c->ws, nres, n)) return rc;
  // The rebased offsets go first, on copy stream 0, from the pinned buffer that also stages the
  // residues.
  rebase_offsets(sh.bind(), offsets + lo, (uint64_t)n + 1, base);
  KMA_HIP(hipMemcpyAsync(c->d_off.p, sh.hoff, off_bytes, hipMemcpyHostToDevice, c->copy[0]));
  if (sh.d_tally) KMA_HIP(hipMemsetAsync(sh.d_tally, 0, n_fid * 4ull, sh.s));
  const double t_setup = ms_since(t_call);
  // Pieces of >= KMA_OPT_HOST_PIECE_MIN residues (default 16 Mi), at most KMA_OPT_HOST_PIECES
  // (default 8; read per call), so a small call is one piece. Streamed calls cut equal pieces:
  // the link does not wait for a piece there, only the kernels do, and a ramp down left kernels
  // queued behind the last copy. Piece-wise (ASCII) calls ramp (plan_pieces).
  const int64_t pm = opt(KMA_OPT_HOST_PIECE_MIN), po = opt(KMA_OPT_HOST_PIECES);
  sh.plan = plan_pieces(sh.hoff, n, nres, pm > 0 ? (uint64_t)pm : 16ull << 20,
                        po > 0 ? (uint64_t)po : 8, /*ramp=*/!sh.packed);
  if (int rc = sh.packed ? sh.stage_streamed() : sh.stage_piecewise()) return rc;
  const Clock::time_point t_o = Clock::now();
  if (int rc = sh.collect_outputs(out_fid + lo, out_count + lo, out_status + lo, tally)) return rc;
  {
    const double p[kProfFields] = {
        t_setup,          sh.t_stage, sh.t_launch, sh.t_wait, ms_since(t_o) - sh.t_wait,
        ms_since(t_call), (double)staging_threads(), (double)sh.plan.n_pieces};
    std::lock_guard<std::mutex> g(g_prof_mu);
    std::copy(p, p + kProfFields, g_prof);
    if (rep < kProfReplicas) std::copy(p, p + kProfFields, g_prof_rep[rep]);
  }
  return KMA_OK;
}
}  // namespace

extern "C" {

// Not in kmeranno.h: measurement hooks (see g_prof). kma_debug_host_profile: the last shard
// call's phases; kma_debug_host_profile_replica: the last shard call of replica `rep` (its index
// in the table's replica list) of a fanned-out host call.
int kma_debug_host_profile(double* out, int n) {
  if (!out || n < 0) return KMA_E_INVALID;
  std::lock_guard<std::mutex> g(g_prof_mu);
  std::copy(g_prof, g_prof + std::min(n, kProfFields), out);
  return KMA_OK;
}
int kma_debug_host_profile_replica(int rep, double* out, int n) {
  if (!out || n < 0 || rep < 0 || rep >= kProfReplicas) return KMA_E_INVALID;
  std::lock_guard<std::mutex> g(g_prof_mu);
  std::copy(g_prof_rep[rep], g_prof_rep[rep] + std::min(n, kProfFields), out);
  return KMA_OK;
}

int kma_workspace_create(int device, kma_workspace** out) {
  if (!out) return fail(KMA_E_INVALID, "null argument");
  DeviceScope ds(device);
  if (ds.err != hipSuccess) return fail(KMA_E_DEVICE, "hipSetDevice(%d)", device);
  kma_workspace* w = new kma_workspace();
  w->device = device;
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
      n_cu > 0)
    w->n_cu = n_cu;
  hipError_t e = hipMalloc(&w->d_gset, 2 * kResPad * 4);  // reserve() grows it
  if (e != hipSuccess) {
    delete w;
    return fail(KMA_E_NOMEM, "workspace: %s", hipGetErrorString(e));
  }
  *out = w;
  return KMA_OK;
}

int kma_workspace_reserve(kma_workspace* ws, uint64_t n_residues) {
  return kma_workspace_reserve_batch(ws, n_residues, n_residues / 16 + 256);
}

int kma_workspace_reserve_batch(kma_workspace* ws, uint64_t n_residues, uint64_t n_seq) {
  if (!ws) return fail(KMA_E_INVALID, "null workspace");
  if (n_residues > kMaxResidues)
    return fail(KMA_E_INVALID, "%llu residues in one call (limit 2^32 - 128)",
                (unsigned long long)n_residues);
  if (n_seq >= (1ull << 31)) return fail(KMA_E_INVALID, "more than 2^31 proteins in one call");
  if (ws->d_gset && n_residues <= ws->res_cap) return KMA_OK;
  DeviceScope ds(ws->device);
  if (ds.err != hipSuccess) return fail(KMA_E_DEVICE, "hipSetDevice(%d)", ws->device);
  free_protein_scratch(ws);
  KMA_HIP(hipMalloc(&ws->d_gset, 2 * (n_residues + kResPad) * 4));
  ws->res_cap = n_residues;
  // The device calls' packed stream (0.625 B per residue), whatever KMA_OPT_PACKED_INPUT is now:
  // a device call that packs must not allocate (it may be graph-captured). Host
  // contexts' workspaces never pack on the device (their calls stage the stream themselves).
  if (!ws->host_ctx) KMA_HIP(hipMalloc(&ws->d_packed, kma::packed_bytes(n_residues + kResPad)));
  return KMA_OK;
}

int kma_workspace_option_set(kma_workspace* ws, int option, int64_t value) {
  if (!ws) return fail(KMA_E_INVALID, "null workspace");
  if (option != KMA_OPT_BLOCK_PROTEINS && option != KMA_OPT_DEFER)
    return fail(KMA_E_INVALID, "option %d is not a workspace option", option);
  if (value != KMA_OPT_DEFAULT && !option_valid(option, value))
    return fail(KMA_E_INVALID, "option %d: value %lld out of range", option, (long long)value);
  (option == KMA_OPT_BLOCK_PROTEINS ? ws->opt_block_proteins : ws->opt_defer) =
      value == KMA_OPT_DEFAULT ? kOptUnset : value;
  return KMA_OK;
}

int kma_workspace_timing(kma_workspace* ws, int enable) {
  if (!ws) return fail(KMA_E_INVALID, "null workspace");
  DeviceScope ds(ws->device);
  if (enable && ws->events.empty()) {
    ws->events.resize(kMaxEv * kTimingRing);
    for (auto& e : ws->events) KMA_HIP(hipEventCreate(&e));
    ws->names.assign(kTimingRing, nullptr);
    ws->n_phases.assign(kTimingRing, 0);
  }
  ws->timing = enable != 0;
  ws->n_timed = 0;
  return KMA_OK;
}

int kma_workspace_phases_read(kma_workspace* ws, uint32_t* n_calls, int* n_phases,
                              double* phase_ms, const char** phase_names) {
  if (!ws || !n_calls || !n_phases || !phase_ms) return fail(KMA_E_INVALID, "null argument");
  DeviceScope ds(ws->device);
  const uint32_t n = std::min(ws->n_timed, kTimingRing);
  *n_calls = 0;
  *n_phases = 0;
  for (int i = 0; i < KMA_MAX_PHASES; ++i) {
    phase_ms[i] = 0.0;
    if (phase_names) phase_names[i] = nullptr;
  }
  if (n == 0) return KMA_OK;
  const uint32_t last = (ws->n_timed - 1) % kTimingRing;  // calls laid out like the last one
  const char* const* names = ws->names[last];
  const int np = ws->n_phases[last];
  for (uint32_t i = 0; i < n; ++i) {
    if (ws->names[i] != names) continue;
    hipEvent_t* e = &ws->events[kMaxEv * i];
    KMA_HIP(hipEventSynchronize(e[np]));
    for (int ph = 0; ph < np; ++ph) {
      float ms = 0;
      KMA_HIP(hipEventElapsedTime(&ms, e[ph], e[ph + 1]));
      phase_ms[ph] += ms;
    }
    ++*n_calls;
  }
  *n_phases = np;
  if (phase_names)
    for (int ph = 0; ph < np; ++ph) phase_names[ph] = names[ph];
  ws->n_timed = 0;
  return KMA_OK;
}

int kma_workspace_timing_read(kma_workspace* ws, uint32_t* n_calls, double* kernel_ms,
                              double* rest_ms) {
  if (!ws || !n_calls || !kernel_ms || !rest_ms) return fail(KMA_E_INVALID, "null argument");
  double ms[KMA_MAX_PHASES];
  const char* names[KMA_MAX_PHASES];
  int np = 0;
  if (int rc = kma_workspace_phases_read(ws, n_calls, &np, ms, names)) return rc;
  // contigs: (probe, scan + emit); proteins: the whole path (every phase), nothing after it
  const bool contigs = np > 0 && names[0] == kContigPhases[0];
  *kernel_ms = 0;
  *rest_ms = 0;
  for (int ph = 0; ph < np; ++ph) (contigs && ph > 0 ? *rest_ms : *kernel_ms) += ms[ph];
  return KMA_OK;
}

int kma_workspace_destroy(kma_workspace* ws) {
  if (!ws) return KMA_OK;
  DeviceScope ds(ws->device);
  for (auto& e : ws->events) (void)hipEventDestroy(e);
  free_protein_scratch(ws);
  free_contig_scratch(ws);
  delete ws;
  return KMA_OK;
}

int kma_annotate_proteins_device(const kma_table* t, kma_workspace* ws, const uint8_t* d_residues,
                                 const uint64_t* d_offsets, uint32_t n_seq, uint64_t n_residues,
                                 int min_hits, uint32_t flags, int32_t* d_fid, int32_t* d_count,
                                 uint8_t* d_status, uint32_t* d_tally, uint32_t n_fid,
                                 void* stream) {
  Replica rep;
  if (int rc = check_device_call(t, ws, d_residues, "residues", d_offsets, n_seq, n_residues,
                                 min_hits, flags, d_fid, d_count, d_status, &rep))
    return rc;
  if (n_seq == 0) return KMA_OK;
  const bool pack = pack_on_device(n_residues);
  if (pack)
    if (int rc = ensure_packed(ws)) return rc;
  DeviceScope ds(rep.device);
  if (ds.err != hipSuccess) return fail(KMA_E_DEVICE, "hipSetDevice(%d)", rep.device);
  return annotate_proteins_on(t, rep, ws, d_residues, d_offsets, n_seq, n_residues, min_hits,
                              flags, d_fid, d_count, d_status, d_tally, n_fid,
                              static_cast<hipStream_t>(stream),
                              pack ? Input::kPackOnDevice : Input::kAscii);
}

uint64_t kma_packed_bytes(uint64_t n_residues) { return kma::packed_bytes(n_residues); }

int kma_pack_residues(const kma_table* t, const uint8_t* residues, uint64_t n, uint8_t* out,
                      uint64_t out_bytes) {
  if ((n && !residues) || !out) return fail(KMA_E_INVALID, "null argument");
  if (out_bytes < kma::packed_bytes(n))
    return fail(KMA_E_CAPACITY, "packed stream of %llu residues needs %llu bytes",
                (unsigned long long)n, (unsigned long long)kma::packed_bytes(n));
  uint8_t std_lut[256];
  if (!t) standard_lut(std_lut);
  const uint8_t* lut = t ? t->lut : std_lut;
  // large streams on the staging pool, in chunks of 2^15 groups (64 residues = 40 bytes each)
  constexpr uint64_t kChunkGroups = 1u << 15;
  const uint64_t n_groups = (n + 63) / 64, n_chunks = (n_groups + kChunkGroups - 1) / kChunkGroups;
  if (n_chunks < 4) {
    kma::pack_residues_host(lut, residues, n, out, out_bytes);
    return KMA_OK;
  }
  staging_pool().run(n_chunks, staging_threads(), [&](uint64_t c) {
    const uint64_t g0 = c * kChunkGroups, g1 = std::min(n_groups, g0 + kChunkGroups);
    const uint64_t r0 = 64 * g0, r1 = std::min(64 * g1, n);
    const uint64_t bytes = g1 == n_groups ? out_bytes - 40 * g0 : 40 * (g1 - g0);
    kma::pack_residues_host(lut, residues + r0, r1 - r0, out + 40 * g0, bytes);
  });
  return KMA_OK;
}

int kma_annotate_packed_device(const kma_table* t, kma_workspace* ws, const uint8_t* d_stream,
                               const uint64_t* d_offsets, uint32_t n_seq, uint64_t n_residues,
                               int min_hits, uint32_t flags, int32_t* d_fid, int32_t* d_count,
                               uint8_t* d_status, uint32_t* d_tally, uint32_t n_fid,
                               void* stream) {
  Replica rep;
  if (int rc = check_device_call(t, ws, d_stream, "stream", d_offsets, n_seq, n_residues,
                                 min_hits, flags, d_fid, d_count, d_status, &rep))
    return rc;
  if (n_seq == 0) return KMA_OK;
  DeviceScope ds(rep.device);
  if (ds.err != hipSuccess) return fail(KMA_E_DEVICE, "hipSetDevice(%d)", rep.device);
  return annotate_proteins_on(t, rep, ws, d_stream, d_offsets, n_seq, n_residues, min_hits, flags,
                              d_fid, d_count, d_status, d_tally, n_fid,
                              static_cast<hipStream_t>(stream), Input::kStream, 0);
}

int kma_annotate_proteins(const kma_table* tc, const uint8_t* residues, const uint64_t* offsets,
                          uint32_t n_seq, int min_hits, uint32_t flags, int32_t* out_fid,
                          int32_t* out_count, uint8_t* out_status, uint32_t* out_tally,
                          uint32_t n_fid) {
  if (int rc = check_protein_call(tc, min_hits, flags)) return rc;
  kma_table* t = const_cast<kma_table*>(tc);  // only the context pool is touched
  if (n_seq == 0) return KMA_OK;
  if (!residues || !offsets || !out_fid || !out_count || !out_status)
    return fail(KMA_E_INVALID, "null argument");
  if (const uint32_t s = offsets_decrease_at(offsets, n_seq); s < n_seq)
    return fail(KMA_E_INVALID, "offsets decrease at %u", s);
  const bool tally = out_tally && n_fid;
  const std::vector<Replica> reps = replicas(t);
  const int nr = (int)std::min<uint64_t>(reps.size(), n_seq);
  const std::vector<uint32_t> b = shard_bounds(offsets, n_seq, nr);
  std::vector<std::vector<uint32_t>> part(tally ? nr : 0, std::vector<uint32_t>(n_fid));
  // A replica's share in slices of at most KMA_OPT_HOST_SLICE residues (default 2^31) of whole
  // proteins, one device call each (the kernels index residues with 32 bits); slice tallies add.
  const int64_t so = opt(KMA_OPT_HOST_SLICE);
  const uint64_t slice = so > 0 ? (uint64_t)so : 1ull << 31;
  const size_t width = staging_width(nr);  // each replica's staging jobs
  const int rc = fan_out(nr, [&](int i) {
    ShardWidth sw(width);
    std::vector<uint32_t> st(tally ? n_fid : 0);
    for (uint32_t lo = b[i]; lo < b[i + 1];) {
      uint32_t hi = (uint32_t)(std::upper_bound(offsets + lo + 1, offsets + b[i + 1] + 1,
                                                offsets[lo] + slice) - offsets) - 1;
      if (hi <= lo) hi = lo + 1;  // one protein longer than a slice: a call of its own
      const bool whole = lo == b[i] && hi == b[i + 1];
      uint32_t* tl = !tally ? nullptr : whole ? part[i].data() : st.data();
      if (int rc = protein_shard(t, reps[i], i, residues, offsets, lo, hi, min_hits, flags,
                                 out_fid, out_count, out_status, tl, n_fid))
        return rc;
      if (tally && !whole)
        for (uint32_t f = 0; f < n_fid; ++f) part[i][f] += st[f];
      lo = hi;
    }
    return (int)KMA_OK;
  });
  if (rc != KMA_OK) return rc;
  for (int i = 0; i < (tally ? nr : 0); ++i)  // the tally reduce of the replicas
    for (uint32_t f = 0; f < n_fid; ++f) out_tally[f] += part[i][f];
  return KMA_OK;
}

}  // extern "C"
