// md5_check.cpp — host check of the MD5 body the device runs per lane (csrc/kma_md5.h: Md5Lane
// begin / load / step, md5_build, md5_transform), built as host code under AddressSanitizer and
// UBSan (Makefile: build/kma_md5_check; tests/test_md5_host.py writes the records with hashlib
// and runs it).
//
//   kma_md5_check RECORDS
//
// RECORDS: per record a u32 flags, a u32 length, the sequence's bytes and the 16 expected digest
// bytes. Every record is hashed at each start alignment 0..7 as the last sequence of a heap
// buffer of exactly (8 + start + length + 32) bytes, the device call's contract (8-byte aligned
// base, 32 readable bytes after the last residue): a read outside it is a sanitizer error.
// All records are then hashed once more as one batch in one such buffer.
//
// The tail words of messages too long to hold (2^29 - 1, 2^29, 2^32 + 5, 2^35 + 3 bytes) are
// checked straight on md5_build, which needs no data, against the padding spelled out bytewise.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/kma_md5.h"

namespace {

struct Record {
  uint32_t flags;
  std::vector<uint8_t> seq;
  uint8_t want[16];
};

bool read_records(const char* path, std::vector<Record>* out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  for (;;) {
    uint32_t head[2];
    if (std::fread(head, 4, 2, f) != 2) break;
    Record r;
    r.flags = head[0];
    r.seq.resize(head[1]);
    if (head[1] && std::fread(r.seq.data(), 1, head[1], f) != head[1]) return std::fclose(f), false;
    if (std::fread(r.want, 1, 16, f) != 16) return std::fclose(f), false;
    out->push_back(std::move(r));
  }
  std::fclose(f);
  return true;
}

void digest_of(const uint8_t* res, uint64_t beg, uint64_t end, uint32_t flags, uint8_t out[16]) {
  uint32_t d[4];
  if (flags & KMA_MD5_UPPER) kma::md5_sequence<true>(res, beg, end, d);
  else kma::md5_sequence<false>(res, beg, end, d);
  std::memcpy(out, d, 16);  // (little-endian host: RFC 1321's byte order)
}

int fail_record(size_t i, const char* what, unsigned align) {
  std::fprintf(stderr, "md5_check: record %zu (%s, start alignment %u): wrong digest\n", i, what,
               align);
  return 1;
}

// Byte j of the padded message of len bytes of zeros, for j >= len - (len % 64) (the tail).
uint8_t padded_byte(uint64_t len, uint64_t j) {
  const uint64_t padded = (len + 8) / 64 * 64 + 64;
  if (j < len) return 0;
  if (j == len) return 0x80;
  if (j < padded - 8) return 0;
  return (uint8_t)((len << 3) >> (8 * (j - (padded - 8))));  // the bit length, little-endian
}

int check_tail(uint64_t len) {
  const uint64_t n_blocks = (len + 8) / 64 + 1;
  const uint64_t first = len / 64;  // the block of the 0x80 byte; one or two blocks to check
  for (uint64_t b = first; b < n_blocks; ++b) {
    uint32_t m[16] = {0};
    const int64_t rem = (int64_t)len - (int64_t)(64 * b);
    kma::md5_build(m, rem, len);
    for (unsigned j = 0; j < 64; ++j) {
      const uint8_t got = (uint8_t)(m[j / 4] >> (8 * (j % 4)));
      if (got != padded_byte(len, 64 * b + j)) {
        std::fprintf(stderr, "md5_check: length %llu block %llu byte %u: %02x\n",
                     (unsigned long long)len, (unsigned long long)b, j, got);
        return 1;
      }
    }
    if ((rem < 56) != (b == n_blocks - 1)) return 1;  // (Md5Lane::step's end of the walk)
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return std::fprintf(stderr, "usage: kma_md5_check RECORDS\n"), 2;
  std::vector<Record> recs;
  if (!read_records(argv[1], &recs) || recs.empty())
    return std::fprintf(stderr, "md5_check: cannot read %s\n", argv[1]), 2;
  size_t hashed = 0;
  for (size_t i = 0; i < recs.size(); ++i) {
    const Record& r = recs[i];
    for (unsigned align = 0; align < 8; ++align) {
      const size_t beg = 8 + align, end = beg + r.seq.size();
      uint8_t* buf = static_cast<uint8_t*>(std::malloc(end + 32));  // (malloc aligns to 16)
      std::memset(buf, 0xA5, end + 32);
      if (!r.seq.empty()) std::memcpy(buf + beg, r.seq.data(), r.seq.size());
      uint8_t got[16];
      digest_of(buf, beg, end, r.flags, got);
      std::free(buf);
      ++hashed;
      if (std::memcmp(got, r.want, 16)) return fail_record(i, "alone", align);
    }
  }
  {  // one batch: every record back to back from byte 8 on
    size_t total = 8;
    for (const Record& r : recs) total += r.seq.size();
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(total + 32));
    std::memset(buf, 0x5A, total + 32);
    size_t at = 8;
    for (const Record& r : recs) {
      if (!r.seq.empty()) std::memcpy(buf + at, r.seq.data(), r.seq.size());
      at += r.seq.size();
    }
    at = 8;
    for (size_t i = 0; i < recs.size(); ++i) {
      uint8_t got[16];
      digest_of(buf, at, at + recs[i].seq.size(), recs[i].flags, got);
      ++hashed;
      if (std::memcmp(got, recs[i].want, 16)) {
        std::free(buf);
        return fail_record(i, "in the batch", (unsigned)(at & 7));
      }
      at += recs[i].seq.size();
    }
    std::free(buf);
  }
  const uint64_t tails[] = {(1ull << 29) - 1, 1ull << 29, (1ull << 32) + 5, (1ull << 35) + 3,
                            55, 56, 63, 64, 119, 120};
  for (uint64_t len : tails)
    if (check_tail(len)) return std::fprintf(stderr, "md5_check: tail of %llu\n",
                                             (unsigned long long)len), 1;
  std::printf("md5_check ok: %zu records, %zu digests, %zu tails\n", recs.size(), hashed,
              sizeof(tails) / sizeof(tails[0]));
  return 0;
}
