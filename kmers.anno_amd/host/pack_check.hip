// pack_check — host check of the device's ASCII -> stream step (kma_device.h: pack8 / store40,
// used by the pack kernel and by the staged probe) against the library's host packer
// (kma_pack_residues): the same stream for every length 0..130 at every misalignment of the
// input, on residues that hold every byte class, with every buffer allocated at its exact size.
// Built with -fsanitize=address,undefined (make build/kma_pack_check); needs no device.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/kma_device.h"
#include "kmeranno.h"

namespace {

// The standard alphabet of kma_pack_residues(table = NULL): 'A'..'Z' -> 1..26, '*' -> 27.
void standard_lut(uint8_t lut[256]) {
  std::memset(lut, 0, 256);
  for (int c = 'A'; c <= 'Z'; ++c) lut[c] = (uint8_t)(c - 'A' + 1);
  lut['*'] = 27;
}

// Byte i of pattern p: letters, or letters mixed with bytes that have no code.
uint8_t residue(int p, uint64_t i) {
  static const uint8_t odd[] = {'*', '7', 'q', 0x00, 0xFF, ' ', '[', '@'};
  const uint8_t letter = (uint8_t)('A' + (i * 7 + (uint64_t)p * 3) % 26);
  switch (p) {
    case 0: return letter;
    case 1: return i % 5 == 2 ? odd[i % 8] : letter;
    case 2: return odd[(i + 3) % 8];  // no letter at all ('*' has a code)
    default: return (i / 8) % 2 ? odd[3 + i % 2] : letter;  // whole groups without a code
  }
}

}  // namespace

int main() {
  uint8_t lut[256];
  standard_lut(lut);
  uint64_t checked = 0;
  for (int p = 0; p < 4; ++p)
    for (uint64_t n = 0; n <= 130; ++n)
      for (uint64_t mis = 0; mis < 8; ++mis) {
        uint8_t* raw = static_cast<uint8_t*>(std::malloc(mis + n ? mis + n : 1));
        uint8_t* in = raw + mis;  // ends with the allocation: a read past n is an error
        for (uint64_t i = 0; i < n; ++i) in[i] = residue(p, i);
        const uint64_t cap = kma_packed_bytes(n), groups = (n + 7) / 8;
        uint8_t* lib = static_cast<uint8_t*>(std::malloc(cap));
        std::memset(lib, 0xA5, cap);
        if (kma_pack_residues(nullptr, in, n, lib, cap) != KMA_OK) {
          std::fprintf(stderr, "kma_pack_residues failed: n=%llu\n", (unsigned long long)n);
          return 1;
        }
        uint8_t* ref = static_cast<uint8_t*>(std::malloc(5 * groups ? 5 * groups : 1));
        for (uint64_t g = 0; g < groups; ++g) {
          uint64_t x = 0;  // residues 8 g .. 8 g + 7, byte j = residue j; past n: byte 0
          for (uint64_t j = 0; j < 8 && 8 * g + j < n; ++j) x |= (uint64_t)in[8 * g + j] << (8 * j);
          kma::store40(ref + 5 * g, kma::pack8(lut, x));
        }
        if (5 * groups > cap || std::memcmp(ref, lib, 5 * groups) != 0) {
          std::fprintf(stderr, "streams differ: pattern %d n=%llu mis=%llu\n", p,
                       (unsigned long long)n, (unsigned long long)mis);
          return 1;
        }
        for (uint64_t i = 5 * groups; i < cap; ++i)
          if (lib[i] != 0) {
            std::fprintf(stderr, "padding not zero: n=%llu byte %llu\n", (unsigned long long)n,
                         (unsigned long long)i);
            return 1;
          }
        std::free(ref);
        std::free(lib);
        std::free(raw);
        ++checked;
      }
  std::printf("pack_check ok: %llu streams\n", (unsigned long long)checked);
  return 0;
}
