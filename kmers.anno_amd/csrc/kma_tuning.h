// kma_tuning.h — the two instrumentation builds of the probe kernels (make variant): their
// device buffers, the macros the kernels write them with and the extern "C" readers. The
// shipped library defines neither switch: every macro below is then empty and no symbol exists.
// The library is not built with relocatable device code, so a buffer belongs to the unit that
// names it: a unit includes this header and, before its namespace, names its reader(s).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#ifdef KMA_BLOCK_CLOCK
// make variant VNAME=clk VFLAGS=-DKMA_BLOCK_CLOCK, scripts/block_clock.py: per block of the
// unit's last probe launch, wall clocks 0..5 at the points its kernel marks (protein probe: 0
// start, 1 records ready, 2 first step matched, 3 steps done, 4 chain walks done, 5 end; 6-frame
// probe: 0 start, 1 tile loaded, 2 translated, 3 bucket loads issued, 4 matched, 5 end); 6
// hardware ids; 7 steps (protein probe). KMA_TUNING_BLOCK_CLOCK(reader): the unit's buffer and
// int reader(uint64_t* out, uint64_t n), which copies its first n words.
#define KMA_TUNING_BLOCK_CLOCK(reader)                                                \
  namespace kma {                                                                     \
  namespace {                                                                         \
  __device__ uint64_t g_block_clk[8 * 65536];                                         \
  }                                                                                   \
  }                                                                                   \
  extern "C" int reader(uint64_t* out, uint64_t n) {                                  \
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(kma::g_block_clk), 8 * n, 0,      \
                                    hipMemcpyDeviceToHost);                           \
  }
#define KMA_CLK_SET(i, v)                                          \
  do {                                                             \
    if (threadIdx.x == 0 && blockIdx.x < 65535)                    \
      g_block_clk[8 * blockIdx.x + (i)] = (v);                     \
  } while (0)
#define KMA_CLK(i) KMA_CLK_SET(i, wall_clock64())
#define KMA_CLK_HW()                                                \
  KMA_CLK_SET(6, (uint64_t)__builtin_amdgcn_s_getreg(20 | (15 << 11)) << 32 | \
                     (uint32_t)__builtin_amdgcn_s_getreg(4 | (31 << 11)))
#else
#define KMA_TUNING_BLOCK_CLOCK(reader)
#define KMA_CLK_SET(i, v) ((void)0)
#define KMA_CLK(i) ((void)0)
#define KMA_CLK_HW() ((void)0)
#endif

#ifdef KMA_TUNE_COUNT
// make variant VNAME=count VFLAGS=-DKMA_TUNE_COUNT, scripts/walk_stats.py: wave-level event
// counts of the protein launches since the last reset: 0 chain flushes, 1 queued walks, 2
// probed windows, 3 home-bucket hits, 4 walk hits, 5 walk hits in the chain's first bucket, 6
// chain buckets loaded by walks, 7 the sum over flush passes of the longest walk (buckets) in
// the pass. KMA_TUNING_WALK_STATS(reader): the buffer and int reader(uint64_t* out, int reset).
#define KMA_TUNING_WALK_STATS(reader)                                                      \
  namespace kma {                                                                          \
  namespace {                                                                              \
  __device__ unsigned long long g_walk_stats[8];                                           \
  }                                                                                        \
  }                                                                                        \
  extern "C" int reader(uint64_t* out, int reset) {                                        \
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(kma::g_walk_stats), 64, 0,          \
                                       hipMemcpyDeviceToHost);                             \
    if (e == hipSuccess && reset) {                                                        \
      const uint64_t z[8] = {};                                                            \
      e = hipMemcpyToSymbol(HIP_SYMBOL(kma::g_walk_stats), z, 64, 0, hipMemcpyHostToDevice); \
    }                                                                                      \
    return (int)e;                                                                         \
  }
#define KMA_COUNT(i, v)                                                                    \
  do {                                                                                     \
    const unsigned long long kma_v_ = (unsigned long long)(v); /* wave-wide, all lanes */  \
    if ((threadIdx.x & 63) == 0)                                                           \
      __hip_atomic_fetch_add(&g_walk_stats[i], kma_v_, __ATOMIC_RELAXED,                   \
                             __HIP_MEMORY_SCOPE_AGENT);                                    \
  } while (0)
// Statements, and a trailing call argument, that exist in a counting build only.
#define KMA_IF_COUNT(...) __VA_ARGS__
#define KMA_COUNT_ARG(x) , x
#else
#define KMA_TUNING_WALK_STATS(reader)
#define KMA_COUNT(i, v) ((void)0)
#define KMA_IF_COUNT(...)
#define KMA_COUNT_ARG(x)
#endif
