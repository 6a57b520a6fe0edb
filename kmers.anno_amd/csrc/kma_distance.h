// kma_distance.h — launcher of the ProteinKmers.distance pair kernel (kma_distance.hip), used by
// kma_abi_sets.cpp; the sets it compares are built by kma_kmersets.hip. Not part of the public
// ABI (see include/kmeranno.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kma {
hipError_t launch_pairs(const uint64_t* sa, const uint64_t* offa, const uint32_t* size_a,
                        const uint64_t* sb, const uint64_t* offb, const uint32_t* size_b,
                        const uint32_t* pa, const uint32_t* pb, uint64_t n_pairs, uint32_t* sim,
                        hipStream_t s);
}  // namespace kma
