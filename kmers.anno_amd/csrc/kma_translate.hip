// kma_translate.hip — protein translation of genome locations on the device.
//
// KmerProcessor.makeFeature (anno/KmerProcessor.java:295-312) ends every kept proposal with
// genome.getDna(loc) and DnaTranslator.pegTranslate(dna, 1, len - 3); both are external to the
// reference and restated in include/kmeranno.h (kma_translate_locations).
//
//   translate_kernel   work is split over the flat output, not over locations: a block owns
//                      kTrTile consecutive residues, a thread four of them (one aligned dword
//                      store; the stream's tail bytewise). The block finds the locations of its
//                      first and last residue once; a thread finds its own by an upper-bound
//                      search of the output offsets inside that range, which steps over runs of
//                      equal offsets (empty locations), and searches again only when its four
//                      residues cross into another location. No thread walks a location's
//                      codons: a 20,000-codon ORF and 20,000 one-codon locations cost the same
//                      per residue.
//
// The base-class table (kma_translate.h; the complement is class ^ 2) and the genetic code live
// in LDS. A streaming pass: 3 byte loads and a third of a dword store per residue.
#include "kma_translate.h"

namespace kma {
namespace {

__global__ __launch_bounds__(kTrBlock) void translate_kernel(TranslateArgs a) {
  __shared__ uint8_t lut[256];
  __shared__ uint8_t code[64];
  __shared__ uint64_t range[2];
  const uint32_t t = threadIdx.x;
  const uint64_t r0 = (uint64_t)blockIdx.x * kTrTile;
  const uint64_t r_end = r0 + kTrTile < a.total ? r0 + kTrTile : a.total;
  lut[t] = tr_base_class(t);
  if (t < 64) code[t] = a.code[t];
  if (t < 2) range[t] = tr_find(a.out_off, 0, a.n_loc - 1, t == 0 ? r0 : r_end - 1);
  __syncthreads();
  tr_thread(a, lut, code, range[0], range[1], r0 + (uint64_t)kTrPerThread * t, r_end);
}

}  // namespace

hipError_t launch_translate(const TranslateArgs& a, hipStream_t stream) {
  const uint64_t blocks = (a.total + kTrTile - 1) / kTrTile;
  hipLaunchKernelGGL(translate_kernel, dim3((unsigned)blocks), dim3(kTrBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace kma
