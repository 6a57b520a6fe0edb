// kma_md5.h — RFC 1321 MD5 of the sequences of a residue batch (kma_md5.hip), shared with the
// C-ABI layer (kma_abi_ops.cpp) and with the host check program (host/md5_check.cpp), which runs
// the same per-block body on the CPU under sanitizers. Not part of the public ABI (see
// include/kmeranno.h, kma_sequence_md5_device).
//
// One lane hashes one sequence: MD5 chains its 64-byte blocks. A lane walks its sequence one
// block per step (Md5Lane::begin, load, step). Every step builds the 16 message words without a
// branch from the bytes left (md5_build: data, the 0x80 byte, zero fill and, in the last block,
// the bit length), so that a lane in the middle of its data, a lane at its tail and a lane at
// the extra padding block of a length with len % 64 >= 56 run the same 64 steps together.
//
// Reads: a sequence starts at any byte. The lane reads the 4-byte aligned words that hold its
// block (16 new ones per block; the 17th is carried from the block before) and funnels
// neighbours by the start's misalignment. A word is read only when it holds a byte of the
// sequence, so nothing before the 4-byte word of the batch's first byte is read; the 16-byte
// groups the words are read in reach at most 15 bytes past the sequence's end.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kmeranno.h"

namespace kma {

// Refill form: waves per compute unit. Fewer waves own longer ranges and lose less to the end of
// a range, where lanes run dry one by one; more waves hide more load latency. Measured on c5's
// batch: 4: 0.28 ms, 8: 0.22 ms, 16: 0.27 ms, 32: 0.31 ms.
constexpr uint32_t kMd5Waves = 8;
constexpr uint32_t kMd5SeqWeight = 64;  // a sequence's fixed share of a wave's range, in bytes

// ({hi, lo} >> sh) as 32 bits, sh = 0, 8, 16 or 24 (v_alignbit on the device).
__host__ __device__ inline uint32_t md5_funnel(uint32_t lo, uint32_t hi, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(hi, lo, sh);
#else
  return sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
#endif
}
__host__ __device__ inline uint32_t md5_rotl(uint32_t x, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(x, x, 32u - s);
#else
  return (x << s) | (x >> (32u - s));
#endif
}
// F, G, H and I of RFC 1321 §3.4 as one 3-input boolean function each: the device's truth
// tables are the expression evaluated on x = 0xF0, y = 0xCC, z = 0xAA (v_bitop3_b32).
template <int Round>
__host__ __device__ inline uint32_t md5_mix(uint32_t x, uint32_t y, uint32_t z) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (Round == 0) return __builtin_amdgcn_bitop3_b32(x, y, z, 0xCA);
  if (Round == 1) return __builtin_amdgcn_bitop3_b32(x, y, z, 0xE4);
  if (Round == 2) return __builtin_amdgcn_bitop3_b32(x, y, z, 0x96);
  return __builtin_amdgcn_bitop3_b32(x, y, z, 0x39);
#else
  if (Round == 0) return (x & y) | (~x & z);
  if (Round == 1) return (x & z) | (y & ~z);
  if (Round == 2) return x ^ y ^ z;
  return y ^ (x | ~z);
#endif
}

#define KMA_MD5_STEP(R, a, b, c, d, k, s, t) \
  a = b + md5_rotl(a + md5_mix<R>(b, c, d) + m[k] + t, s)

// One block into the state: the 64 steps written out, every m[] index a literal.
__host__ __device__ inline void md5_transform(uint32_t (&h)[4], const uint32_t (&m)[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
  KMA_MD5_STEP(0, a, b, c, d, 0, 7, 0xd76aa478u);
  KMA_MD5_STEP(0, d, a, b, c, 1, 12, 0xe8c7b756u);
  KMA_MD5_STEP(0, c, d, a, b, 2, 17, 0x242070dbu);
  KMA_MD5_STEP(0, b, c, d, a, 3, 22, 0xc1bdceeeu);
  KMA_MD5_STEP(0, a, b, c, d, 4, 7, 0xf57c0fafu);
  KMA_MD5_STEP(0, d, a, b, c, 5, 12, 0x4787c62au);
  KMA_MD5_STEP(0, c, d, a, b, 6, 17, 0xa8304613u);
  KMA_MD5_STEP(0, b, c, d, a, 7, 22, 0xfd469501u);
  KMA_MD5_STEP(0, a, b, c, d, 8, 7, 0x698098d8u);
  KMA_MD5_STEP(0, d, a, b, c, 9, 12, 0x8b44f7afu);
  KMA_MD5_STEP(0, c, d, a, b, 10, 17, 0xffff5bb1u);
  KMA_MD5_STEP(0, b, c, d, a, 11, 22, 0x895cd7beu);
  KMA_MD5_STEP(0, a, b, c, d, 12, 7, 0x6b901122u);
  KMA_MD5_STEP(0, d, a, b, c, 13, 12, 0xfd987193u);
  KMA_MD5_STEP(0, c, d, a, b, 14, 17, 0xa679438eu);
  KMA_MD5_STEP(0, b, c, d, a, 15, 22, 0x49b40821u);

  KMA_MD5_STEP(1, a, b, c, d, 1, 5, 0xf61e2562u);
  KMA_MD5_STEP(1, d, a, b, c, 6, 9, 0xc040b340u);
  KMA_MD5_STEP(1, c, d, a, b, 11, 14, 0x265e5a51u);
  KMA_MD5_STEP(1, b, c, d, a, 0, 20, 0xe9b6c7aau);
  KMA_MD5_STEP(1, a, b, c, d, 5, 5, 0xd62f105du);
  KMA_MD5_STEP(1, d, a, b, c, 10, 9, 0x02441453u);
  KMA_MD5_STEP(1, c, d, a, b, 15, 14, 0xd8a1e681u);
  KMA_MD5_STEP(1, b, c, d, a, 4, 20, 0xe7d3fbc8u);
  KMA_MD5_STEP(1, a, b, c, d, 9, 5, 0x21e1cde6u);
  KMA_MD5_STEP(1, d, a, b, c, 14, 9, 0xc33707d6u);
  KMA_MD5_STEP(1, c, d, a, b, 3, 14, 0xf4d50d87u);
  KMA_MD5_STEP(1, b, c, d, a, 8, 20, 0x455a14edu);
  KMA_MD5_STEP(1, a, b, c, d, 13, 5, 0xa9e3e905u);
  KMA_MD5_STEP(1, d, a, b, c, 2, 9, 0xfcefa3f8u);
  KMA_MD5_STEP(1, c, d, a, b, 7, 14, 0x676f02d9u);
  KMA_MD5_STEP(1, b, c, d, a, 12, 20, 0x8d2a4c8au);

  KMA_MD5_STEP(2, a, b, c, d, 5, 4, 0xfffa3942u);
  KMA_MD5_STEP(2, d, a, b, c, 8, 11, 0x8771f681u);
  KMA_MD5_STEP(2, c, d, a, b, 11, 16, 0x6d9d6122u);
  KMA_MD5_STEP(2, b, c, d, a, 14, 23, 0xfde5380cu);
  KMA_MD5_STEP(2, a, b, c, d, 1, 4, 0xa4beea44u);
  KMA_MD5_STEP(2, d, a, b, c, 4, 11, 0x4bdecfa9u);
  KMA_MD5_STEP(2, c, d, a, b, 7, 16, 0xf6bb4b60u);
  KMA_MD5_STEP(2, b, c, d, a, 10, 23, 0xbebfbc70u);
  KMA_MD5_STEP(2, a, b, c, d, 13, 4, 0x289b7ec6u);
  KMA_MD5_STEP(2, d, a, b, c, 0, 11, 0xeaa127fau);
  KMA_MD5_STEP(2, c, d, a, b, 3, 16, 0xd4ef3085u);
  KMA_MD5_STEP(2, b, c, d, a, 6, 23, 0x04881d05u);
  KMA_MD5_STEP(2, a, b, c, d, 9, 4, 0xd9d4d039u);
  KMA_MD5_STEP(2, d, a, b, c, 12, 11, 0xe6db99e5u);
  KMA_MD5_STEP(2, c, d, a, b, 15, 16, 0x1fa27cf8u);
  KMA_MD5_STEP(2, b, c, d, a, 2, 23, 0xc4ac5665u);

  KMA_MD5_STEP(3, a, b, c, d, 0, 6, 0xf4292244u);
  KMA_MD5_STEP(3, d, a, b, c, 7, 10, 0x432aff97u);
  KMA_MD5_STEP(3, c, d, a, b, 14, 15, 0xab9423a7u);
  KMA_MD5_STEP(3, b, c, d, a, 5, 21, 0xfc93a039u);
  KMA_MD5_STEP(3, a, b, c, d, 12, 6, 0x655b59c3u);
  KMA_MD5_STEP(3, d, a, b, c, 3, 10, 0x8f0ccc92u);
  KMA_MD5_STEP(3, c, d, a, b, 10, 15, 0xffeff47du);
  KMA_MD5_STEP(3, b, c, d, a, 1, 21, 0x85845dd1u);
  KMA_MD5_STEP(3, a, b, c, d, 8, 6, 0x6fa87e4fu);
  KMA_MD5_STEP(3, d, a, b, c, 15, 10, 0xfe2ce6e0u);
  KMA_MD5_STEP(3, c, d, a, b, 6, 15, 0xa3014314u);
  KMA_MD5_STEP(3, b, c, d, a, 13, 21, 0x4e0811a1u);
  KMA_MD5_STEP(3, a, b, c, d, 4, 6, 0xf7537e82u);
  KMA_MD5_STEP(3, d, a, b, c, 11, 10, 0xbd3af235u);
  KMA_MD5_STEP(3, c, d, a, b, 2, 15, 0x2ad7d2bbu);
  KMA_MD5_STEP(3, b, c, d, a, 9, 21, 0xeb86d391u);
  h[0] += a;
  h[1] += b;
  h[2] += c;
  h[3] += d;
}
#undef KMA_MD5_STEP

// a..z -> A..Z in each byte of x, no other byte touched (KMA_MD5_UPPER). Per byte on its low 7
// bits: + 0x1F carries into bit 7 from 'a' up, + 0x05 from '{' up; bytes >= 0x80 are excluded.
__host__ __device__ inline uint32_t md5_upper(uint32_t x) {
  const uint32_t low = x & 0x7F7F7F7Fu;
  const uint32_t ge_a = low + 0x1F1F1F1Fu, gt_z = low + 0x05050505u;
  return x ^ ((ge_a & ~gt_z & ~x & 0x80808080u) >> 2);
}

// The message words of one block, in place. On entry m[i] holds the bytes 4 i .. 4 i + 3 of the
// block, little-endian (anything where the message has ended); rem = message bytes from the
// block's first byte on: > 0 inside the data, 0 when the data ended exactly at the block before,
// negative in the extra block of a message whose 0x80 byte stands in the block before. The
// block is the message's last iff rem < 56; it then carries the bit length 8 len in words 14
// and 15, which the byte rule has zeroed. No branch: every word is a select on rem - 4 i.
__host__ __device__ inline void md5_build(uint32_t (&m)[16], int64_t rem, uint64_t len) {
  const int32_t r = rem > 64 ? 64 : rem < -1 ? -1 : (int32_t)rem;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int32_t t = r - 4 * i;  // data bytes of the message from this word on
    const uint32_t sh = ((uint32_t)t & 3u) * 8u;
    const uint32_t edge = (m[i] & ~(~0u << sh)) | (0x80u << sh);  // t data bytes, then 0x80
    m[i] = t >= 4 ? m[i] : t < 0 ? 0u : edge;
  }
  const bool last = rem < 56;
  m[14] |= last ? (uint32_t)(len << 3) : 0u;
  m[15] |= last ? (uint32_t)(len >> 29) : 0u;
}

// One lane's walk over one sequence.
struct Md5Lane {
  uint32_t h[4];
  uint32_t carry;     // the aligned word that holds the next block's first byte
  uint32_t sh;        // 8 * (the start's address mod 4)
  const uint32_t* q;  // that word's address
  int64_t rem;        // md5_build's rem of the next block
  uint64_t len;

  // Sequence bytes [beg, end) of res.
  __host__ __device__ void begin(const uint8_t* res, uint64_t beg, uint64_t end) {
    h[0] = 0x67452301u;
    h[1] = 0xefcdab89u;
    h[2] = 0x98badcfeu;
    h[3] = 0x10325476u;
    len = end - beg;
    rem = (int64_t)len;
    const uint8_t* p = res + beg;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
    sh = mis * 8u;
    q = reinterpret_cast<const uint32_t*>(p - mis);  // (stepped back from res: a global pointer)
    carry = len ? q[0] : 0u;
  }
  // How many of the 16 words after q hold a byte of the sequence (the block's and the next
  // block's first): word 1 + k starts 4 - sh / 8 + 4 k bytes into what is left.
  __host__ __device__ uint32_t words_needed() const {
    const int64_t past = rem - (int64_t)(4u - sh / 8u);  // bytes left from word 1 on
    return past <= 0 ? 0u : past >= 64 ? 16u : (uint32_t)((past + 3) >> 2);
  }
  // The 16 words after q, in groups of four, each group read iff its first word is needed.
  __host__ __device__ void load(uint32_t (&w)[16]) const {
    const uint32_t n = words_needed();
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0;
      if ((uint32_t)(4 * g) < n) {
        const uint32_t* s = q + 1 + 4 * g;
        v0 = s[0], v1 = s[1], v2 = s[2], v3 = s[3];
      }
      w[4 * g] = v0, w[4 * g + 1] = v1, w[4 * g + 2] = v2, w[4 * g + 3] = v3;
    }
  }
  // One block from the 16 words after q. True when it was the sequence's last: h is the digest
  // (h[0] first, each word little-endian, is RFC 1321's byte order).
  template <bool Upper>
  __host__ __device__ bool step(const uint32_t (&w)[16]) {
    uint32_t m[16];
    m[0] = md5_funnel(carry, w[0], sh);
#pragma unroll
    for (int i = 1; i < 16; ++i) m[i] = md5_funnel(w[i - 1], w[i], sh);
    if (Upper) {
#pragma unroll
      for (int i = 0; i < 16; ++i) m[i] = md5_upper(m[i]);
    }
    md5_build(m, rem, len);
    md5_transform(h, m);
    const bool last = rem < 56;
    carry = w[15];
    q += 16;
    rem -= 64;
    return last;
  }
};

// The whole walk of one sequence, as the kernel's loop strings it together per lane (the host
// check program runs this).
template <bool Upper>
__host__ __device__ inline void md5_sequence(const uint8_t* res, uint64_t beg, uint64_t end,
                                             uint32_t (&digest)[4]) {
  Md5Lane l;
  l.begin(res, beg, end);
  uint32_t w[16];
  do l.load(w);
  while (!l.step<Upper>(w));
  for (int i = 0; i < 4; ++i) digest[i] = l.h[i];
}

struct Md5Args {
  const uint8_t* res;    // sequence s is res[off[s] .. off[s + 1]); 4-byte aligned
  const uint64_t* off;   // n_seq + 1
  uint32_t n_seq;        // > 0
  uint32_t n_waves;      // the grid (one wave per block)
  uint32_t upper;        // KMA_MD5_UPPER
  uint4* digest;         // n_seq
};
// Kernel forms (kma_md5.hip). The shipped call uses kMd5Default; the others exist for the
// measurement of DESIGN.md §5.9 (kma_debug_sequence_md5_device).
constexpr uint32_t kMd5Static = 1;  // lane i takes sequence i of 64; no refill
constexpr uint32_t kMd5Coop = 2;    // 16 lanes fetch one sequence's block through LDS
constexpr uint32_t kMd5Default = 0;
// The grid the form uses for n_seq sequences on a device of n_cu compute units.
uint32_t md5_waves(uint32_t n_seq, uint32_t form, uint32_t n_cu, uint32_t waves_per_cu);
hipError_t launch_md5(const Md5Args& a, uint32_t form, hipStream_t stream);

// ---- duplicate grouping over the digests (kma_check_sequences) ---------------------------------
struct SeqCheckArgs {
  const uint4* digest;   // n
  const uint64_t* off;   // n + 1 (an empty sequence joins no group)
  const uint32_t* fun;   // n, or null
  uint32_t n;
  uint64_t *key_a, *key_b;   // n each
  uint32_t *idx_a, *idx_b;   // n each
  uint32_t *start;           // n: sorted position of the head of the position's run
  uint32_t *count, *fmin, *fmax;  // n each, at run heads
  int32_t* rep;          // outputs, n each
  uint32_t* size;
  uint8_t* mixed;
  uint64_t* stats;       // 3
};
// temp == nullptr: *temp_bytes = the need. Otherwise the sorts, run heads and per-run reductions
// on `stream`.
hipError_t launch_seq_check(const SeqCheckArgs& a, void* temp, size_t* temp_bytes,
                            hipStream_t stream);

}  // namespace kma
