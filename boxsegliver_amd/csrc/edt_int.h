// The integer core of the exact squared Euclidean distance transforms, shared by slice_prior.hip and
// weights.hip: the nearest set bit of a bit row for the first axis, a brute-force minimum for every other.  int32 throughout.
#pragma once
#include "common.h"

constexpr int IEDT_NONE = 1 << 30;        // "no site on this line": a minimum that is still >= IEDT_NONE has seen no site at all
constexpr int IEDT_STAGE = 128;           // rows of a 64-column strip staged at a time: 32 KiB of LDS
constexpr int IEDT_T = 16;                // outputs along the axis of a block of iedt_axis_min: four per thread
constexpr int IEDT_MAX_BITS = 4096;       // the longest bit row: 64 words
// no term of iedt_axis_min overflows int32, outputs up to IEDT_T - 1 past the end of the axis (computed, never stored) included
constexpr bool iedt_fits(int64_t scale, int64_t L) { return IEDT_NONE + scale * (L + IEDT_T - 2) * (L + IEDT_T - 2) < ((int64_t)1 << 31); }

// The distance from x to the nearest set bit of bits[0 .. nwords) (bit b of word w is element 64 w + b), or -1 without one.
__device__ __forceinline__ int iedt_nearest_bit(const unsigned long long* bits, int nwords, int x) {
  const int w = x >> 6, l = x & 63;
  int g = -1, ww = w;
  unsigned long long m = bits[w] & (~0ull >> (63 - l));        // the nearest site at or left of x: x's own word, then word by word
  while (m == 0 && ww > 0) m = bits[--ww];
  if (m != 0) g = x - (ww * 64 + 63 - __clzll((long long)m));
  m = bits[w] & (~0ull << l);                                  // at or right of x
  ww = w;
  while (m == 0 && ww + 1 < nwords) m = bits[++ww];
  if (m == 0) return g;
  const int r = ww * 64 + __ffsll((long long)m) - 1 - x;
  return g < 0 ? r : min(g, r);
}

// best[k] = min over j in [0, L) of scale * (i0 + k - j)^2 + col[j * stride], k = 0 .. 3, in every thread of a 256-thread block
// (all of them call: it synchronises).  The thread's column is lane threadIdx.x & 63 of a 64-column strip and col its element
// j = 0, read only where `live` (a dead column stages IEDT_NONE); wave w passes i0 = t0 + 4 w.  The strip goes through `stage`
// IEDT_STAGE rows at a time, a lane per column: each LDS row is read conflict-free, and one read serves the four outputs.
__device__ __forceinline__ void iedt_axis_min(int (&stage)[IEDT_STAGE][64], const int32_t* __restrict__ col, bool live, int64_t stride,
                                              int L, int i0, int scale, int (&best)[4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  best[0] = best[1] = best[2] = best[3] = IEDT_NONE;
  for (int c0 = 0; c0 < L; c0 += IEDT_STAGE) {
    const int rows = min(IEDT_STAGE, L - c0);
    if (c0 > 0) __syncthreads();                               // the chunk before has been read
    for (int r = wave; r < rows; r += 4) stage[r][lane] = live ? col[(int64_t)(c0 + r) * stride] : IEDT_NONE;
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      const int v = stage[r][lane], di = i0 - (c0 + r);
#pragma unroll
      for (int k = 0; k < 4; ++k) best[k] = min(best[k], scale * (di + k) * (di + k) + v);
    }
  }
}
