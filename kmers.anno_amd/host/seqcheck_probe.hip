// seqcheck_probe — runs the duplicate grouping of kma_check_sequences (kma::launch_seq_check,
// csrc/kma_md5.hip) on digests given by the caller instead of computed ones.
//
//   kma_seqcheck_probe RECORDS OUT
//
// Why: through kma_check_sequences the grouping only ever sees real MD5 digests, and two of
// those never agree in one 64-bit half. The properties of the 128-bit sort and of the run heads
// (digests that share a half, a word or all but one bit are different groups) need digests
// that are chosen. The program links build/kma_md5.o, the object that libkmeranno.so ships, so
// the launcher and the sc_* kernels run unmodified; it is a test program and no part of the
// library or its ABI. tests/test_gpu_seqcheck_scale.py writes the records (tests/
// seqcheck_cases.py) and compares OUT with a dict grouping.
//
// RECORDS (little-endian), any number of records, each:
//   u32 n           sequences, 1 .. 2^31 - 1
//   u32 has_fun     0 or 1
//   n x 16 bytes    the digests (uint4 x, y, z, w in this byte order: bytes 0..7 are the low
//                   half of the sort key, bytes 8..15 the high half)
//   n x u32         lengths; only zero against non-zero matters (an empty sequence joins no
//                   group). They become the n + 1 offsets the launcher reads.
//   n x u32         function ids, present iff has_fun
// OUT, per record: u32 n, n x i32 rep, n x u32 size, n x u8 mixed, 3 x u64 stats.
//
// Precondition, the caller's: no non-empty entry of a record carries the digest of an empty
// one. sc_reduce and sc_emit skip empty sequences by length and take a run's head by position;
// for real MD5 the empty message's digest belongs to empty sequences alone, and the kernels
// rely on that.
//
// Per record the device buffers are those of kma_check_sequences (one hipMalloc each, the same
// sizes), the temp size is asked for first, and the launcher runs on the null stream. One
// process handles the whole file. Every HIP status is checked: the first failure prints the call
// and ends the process with status 1 before anything else is launched. A malformed file is
// status 2, before the device is touched.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/kma_md5.h"

#define HIP_OK(call)                                                                         \
  do {                                                                                       \
    const hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                                  \
      std::fprintf(stderr, "seqcheck_probe: record %zu: %s: %s\n", g_record, #call,          \
                   hipGetErrorString(e_));                                                   \
      std::exit(1);                                                                          \
    }                                                                                        \
  } while (0)

namespace {

size_t g_record = 0;

struct Record {
  uint32_t n = 0;
  const uint8_t* digest = nullptr;  // n x 16
  const uint8_t* length = nullptr;  // n x u32
  const uint8_t* fun = nullptr;     // n x u32, or null
};

[[noreturn]] void malformed(const char* what) {
  std::fprintf(stderr, "seqcheck_probe: record %zu: %s\n", g_record, what);
  std::exit(2);
}

// The records of the file, each checked against the bytes that are there.
std::vector<Record> parse(const std::vector<uint8_t>& file) {
  std::vector<Record> out;
  size_t at = 0;
  while (at < file.size()) {
    g_record = out.size();
    if (file.size() - at < 8) malformed("truncated header");
    uint32_t n, has_fun;
    std::memcpy(&n, &file[at], 4);
    std::memcpy(&has_fun, &file[at + 4], 4);
    at += 8;
    if (n == 0 || n >= (1u << 31)) malformed("n outside 1 .. 2^31 - 1");
    if (has_fun > 1) malformed("has_fun is neither 0 nor 1");
    const size_t need = (size_t)n * (has_fun ? 24u : 20u);
    if (file.size() - at < need) malformed("truncated body");
    Record r;
    r.n = n;
    r.digest = &file[at];
    r.length = r.digest + (size_t)n * 16;
    r.fun = has_fun ? r.length + (size_t)n * 4 : nullptr;
    at += need;
    out.push_back(r);
  }
  return out;
}

template <class T>
T* dev_alloc(size_t bytes) {
  void* p = nullptr;
  HIP_OK(hipMalloc(&p, bytes ? bytes : 1));
  return static_cast<T*>(p);
}

void run(const Record& r, std::FILE* out) {
  const size_t n = r.n;
  std::vector<uint64_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    uint32_t len;
    std::memcpy(&len, r.length + 4 * i, 4);
    off[i + 1] = off[i] + len;
  }
  std::vector<void*> owned;
  auto own = [&owned](auto* p) {
    owned.push_back(p);
    return p;
  };
  uint4* d_digest = own(dev_alloc<uint4>(n * 16));
  uint64_t* d_off = own(dev_alloc<uint64_t>((n + 1) * 8));
  uint32_t* d_fun = r.fun ? own(dev_alloc<uint32_t>(n * 4)) : nullptr;
  kma::SeqCheckArgs a{};
  for (uint64_t** p : {&a.key_a, &a.key_b}) *p = own(dev_alloc<uint64_t>(n * 8));
  for (uint32_t** p : {&a.idx_a, &a.idx_b, &a.start, &a.count, &a.fmin, &a.fmax, &a.size})
    *p = own(dev_alloc<uint32_t>(n * 4));
  a.rep = own(dev_alloc<int32_t>(n * 4));
  a.mixed = own(dev_alloc<uint8_t>(n));
  a.stats = own(dev_alloc<uint64_t>(24));
  a.digest = d_digest;
  a.off = d_off;
  a.fun = d_fun;
  a.n = r.n;
  HIP_OK(hipMemcpy(d_digest, r.digest, n * 16, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_off, off.data(), (n + 1) * 8, hipMemcpyHostToDevice));
  if (d_fun) HIP_OK(hipMemcpy(d_fun, r.fun, n * 4, hipMemcpyHostToDevice));

  size_t temp_bytes = 0;
  HIP_OK(kma::launch_seq_check(a, nullptr, &temp_bytes, nullptr));
  void* temp = own(dev_alloc<uint8_t>(temp_bytes));
  size_t given = temp_bytes;
  HIP_OK(kma::launch_seq_check(a, temp, &given, nullptr));
  HIP_OK(hipDeviceSynchronize());

  std::vector<int32_t> rep(n);
  std::vector<uint32_t> size(n);
  std::vector<uint8_t> mixed(n);
  uint64_t stats[3];
  HIP_OK(hipMemcpy(stats, a.stats, 24, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(rep.data(), a.rep, n * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(size.data(), a.size, n * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(mixed.data(), a.mixed, n, hipMemcpyDeviceToHost));
  for (void* p : owned) HIP_OK(hipFree(p));

  const bool ok = std::fwrite(&r.n, 4, 1, out) == 1 && std::fwrite(rep.data(), 4, n, out) == n &&
                  std::fwrite(size.data(), 4, n, out) == n &&
                  std::fwrite(mixed.data(), 1, n, out) == n && std::fwrite(stats, 8, 3, out) == 3;
  if (!ok) {
    std::fprintf(stderr, "seqcheck_probe: record %zu: short write\n", g_record);
    std::exit(1);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s RECORDS OUT\n", argv[0]);
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) {
    std::perror(argv[1]);
    return 2;
  }
  std::vector<uint8_t> file;
  uint8_t buf[1 << 16];
  for (size_t got; (got = std::fread(buf, 1, sizeof buf, in)) > 0;)
    file.insert(file.end(), buf, buf + got);
  std::fclose(in);
  const std::vector<Record> records = parse(file);
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) {
    std::perror(argv[2]);
    return 2;
  }
  for (g_record = 0; g_record < records.size(); ++g_record) run(records[g_record], out);
  if (std::fclose(out) != 0) {
    std::perror(argv[2]);
    return 1;
  }
  std::printf("seqcheck_probe ok: %zu records\n", records.size());
  return 0;
}
