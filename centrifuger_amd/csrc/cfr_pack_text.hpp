// cfr_pack_text.hpp — the 2-bit text of the index writer: the packing kernel and the readers the device files of the writer share
// (cfr_build_sa.hip, cfr_refseq.hip).  2 bits per symbol, the first symbol of a word in its top bits.  Internal, HIP only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace cfr {
namespace {

// ASCII text (a piece starting at a multiple of 32) -> packed words; *bad is raised when a character is not an upper-case A,C,G,T
__global__ void k_pack_text(const uint8_t *text, uint64_t count, uint64_t *words, unsigned int *bad) {
  const uint64_t wI = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (wI * 32 >= count) return;
  uint64_t w = 0;
  const uint64_t base = wI * 32;
  for (uint32_t k = 0; k < 32 && base + k < count; ++k) {
    const uint32_t ch = text[base + k];
    const uint32_t c = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
    if (c > 3u) *bad = 1u;
    w |= (uint64_t)(c & 3u) << (62 - 2 * k);
  }
  words[wI] = w;
}
// the 32 symbols from pos on, the first one in the top bits (reads the word behind the one pos lies in)
__device__ __forceinline__ uint64_t key32(const uint64_t *T, uint64_t pos) {
  const uint32_t o = (uint32_t)pos & 31u;
  const uint64_t w0 = T[pos >> 5];
  if (o == 0) return w0;
  return (w0 << (2 * o)) | (T[(pos >> 5) + 1] >> (64 - 2 * o));
}
__device__ __forceinline__ uint32_t sym_at(const uint64_t *T, uint64_t pos) { return (uint32_t)(T[pos >> 5] >> (62 - 2 * (pos & 31))) & 3u; }

}  // namespace
}  // namespace cfr
