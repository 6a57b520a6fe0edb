// pack_check — host check of the device's ASCII -> stream step (kma_device.h: pack8 / store40,
// used by the pack kernel and by the staged probe) against the host packer (kma_pack.cpp:
// kma::pack_residues_host, compiled into this program so that its AVX2 code is instrumented too,
// and kma_pack_residues of the library): the same stream
//   - for every length 0..130 at every misalignment of the input, with the standard alphabet and
//     with one and four extra table symbols (codes 28..31, a lower-case letter and a byte >= 128
//     among them), on residues that hold every byte class;
//   - for lengths around the 512-residue blocks of the non-temporal path (511, 512, 513, 1061,
//     4101), into outputs that are 64-byte aligned (that path) and misaligned (the plain one);
// with every buffer allocated at its exact size.
// Built with -fsanitize=address,undefined (make build/kma_pack_check); needs no device.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/kma_device.h"
#include "../csrc/kma_pack.h"
#include "kmeranno.h"

namespace {

// The standard alphabet of kma_pack_residues(table = NULL): 'A'..'Z' -> 1..26, '*' -> 27; then
// the first n_extra bytes of "-1a\xC3" -> 28.. in byte order, as a table's creator numbers them.
void make_lut(uint8_t lut[256], int n_extra) {
  static const uint8_t extra[4] = {'-', '1', 'a', 0xC3};
  std::memset(lut, 0, 256);
  for (int c = 'A'; c <= 'Z'; ++c) lut[c] = (uint8_t)(c - 'A' + 1);
  lut['*'] = 27;
  for (int i = 0; i < n_extra; ++i) lut[extra[i]] = (uint8_t)(28 + i);
}

constexpr int kPatterns = 5;

// Byte i of pattern p: letters, letters mixed with bytes that have no code, or every byte value.
uint8_t residue(int p, uint64_t i) {
  static const uint8_t odd[] = {'*', '7', 'q', 0x00, 0xFF, ' ', '[', '@'};
  const uint8_t letter = (uint8_t)('A' + (i * 7 + (uint64_t)p * 3) % 26);
  switch (p) {
    case 0: return letter;
    case 1: return i % 5 == 2 ? odd[i % 8] : letter;
    case 2: return odd[(i + 3) % 8];  // no letter at all ('*' has a code)
    case 3: return (i / 8) % 2 ? odd[3 + i % 2] : letter;  // whole groups without a code
    default: return (uint8_t)(i * 101 + 7);  // all 256 byte values in every 256 residues
  }
}

uint64_t checked = 0;

// One input of n residues at misalignment in_mis, packed into an output of exactly
// kma_packed_bytes(n) bytes that starts out_off bytes past a 64-byte boundary: by
// kma::pack_residues_host with `lut`, and (through_library) by kma_pack_residues with the standard
// alphabet; each against pack8 / store40 with the same LUT.
bool check(const uint8_t* lut, bool through_library, int p, uint64_t n, uint64_t in_mis,
           uint64_t out_off) {
  uint8_t* raw = static_cast<uint8_t*>(std::malloc(in_mis + n ? in_mis + n : 1));
  uint8_t* in = raw + in_mis;  // ends with the allocation: a read past n is an error
  for (uint64_t i = 0; i < n; ++i) in[i] = residue(p, i);
  const uint64_t cap = kma_packed_bytes(n), groups = (n + 7) / 8;
  uint8_t* ref = static_cast<uint8_t*>(std::malloc(5 * groups ? 5 * groups : 1));
  for (uint64_t g = 0; g < groups; ++g) {
    uint64_t x = 0;  // residues 8 g .. 8 g + 7, byte j = residue j; past n: byte 0
    for (uint64_t j = 0; j < 8 && 8 * g + j < n; ++j) x |= (uint64_t)in[8 * g + j] << (8 * j);
    kma::store40(ref + 5 * g, kma::pack8(lut, x));
  }
  bool ok = 5 * groups <= cap;
  for (int pass = 0; ok && pass < (through_library ? 2 : 1); ++pass) {
    void* mem = nullptr;
    if (posix_memalign(&mem, 64, out_off + cap) != 0) return false;
    uint8_t* out = static_cast<uint8_t*>(mem) + out_off;  // ends with the allocation
    std::memset(out, 0xA5, cap);
    if (pass == 0) {
      kma::pack_residues_host(lut, in, n, out, cap);
    } else if (kma_pack_residues(nullptr, in, n, out, cap) != KMA_OK) {
      std::fprintf(stderr, "kma_pack_residues failed: n=%llu\n", (unsigned long long)n);
      ok = false;
    }
    if (ok && std::memcmp(ref, out, 5 * groups) != 0) {
      std::fprintf(stderr, "streams differ (%s): pattern %d n=%llu in+%llu out+%llu\n",
                   pass ? "library" : "direct", p, (unsigned long long)n,
                   (unsigned long long)in_mis, (unsigned long long)out_off);
      ok = false;
    }
    for (uint64_t i = 5 * groups; ok && i < cap; ++i)
      if (out[i] != 0) {
        std::fprintf(stderr, "padding not zero: n=%llu byte %llu\n", (unsigned long long)n,
                     (unsigned long long)i);
        ok = false;
      }
    std::free(mem);
    ++checked;
  }
  std::free(ref);
  std::free(raw);
  return ok;
}

}  // namespace

int main() {
  static const int extras[] = {0, 1, 4};
  static const uint64_t longs[] = {511, 512, 513, 1024 + 37, 4096 + 5};
  static const uint64_t out_offs[] = {0, 1, 32};  // 0: the non-temporal path from 512 residues on
  for (int e = 0; e < 3; ++e) {
    uint8_t lut[256];
    make_lut(lut, extras[e]);
    const bool std_lut = extras[e] == 0;
    for (int p = 0; p < kPatterns; ++p) {
      for (uint64_t n = 0; n <= 130; ++n)
        for (uint64_t mis = 0; mis < 8; ++mis)  // outputs at 64-byte boundaries and 8..56 past one
          if (!check(lut, std_lut, p, n, mis, mis % 2 ? 8 * mis : 0)) return 1;
      for (uint64_t n : longs)
        for (uint64_t off : out_offs)
          for (uint64_t mis = 0; mis < 6; mis += 5)
            if (!check(lut, std_lut, p, n, mis, off)) return 1;
    }
  }
  std::printf("pack_check ok: %llu streams\n", (unsigned long long)checked);
  return 0;
}
