// Bit-set searches over a sentence's columns, one 64-bit word per 64 columns (wave ballots parked in the LDS): shared by the
// chunk-counting kernel (entity.hip) and the chunk-emitting kernel (crf_entities.hip).
#pragma once
#include "common.h"

namespace mtvaf {

// greatest set bit of `bits` strictly below column c (le: at or below), or -1
__device__ __forceinline__ int ent_prev(const uint64_t* bits, int c, bool le) {
  int w = c >> 6;
  const int b = c & 63;
  uint64_t m = bits[w] & (le ? (2ull << b) - 1 : (1ull << b) - 1);  // b == 63: 2 << 63 wraps to 0, minus 1 = all ones
  for (;;) {
    if (m) return 64 * w + 63 - __clzll((long long)m);
    if (--w < 0) return -1;
    m = bits[w];
  }
}
// lowest set bit strictly above column c among the first W words, or -1
__device__ __forceinline__ int ent_next(const uint64_t* bits, int c, int W) {
  int w = c >> 6;
  const int b = c & 63;
  uint64_t m = bits[w] & ~((2ull << b) - 1);
  for (;;) {
    if (m) return 64 * w + __ffsll((long long)m) - 1;
    if (++w >= W) return -1;
    m = bits[w];
  }
}

}  // namespace mtvaf
