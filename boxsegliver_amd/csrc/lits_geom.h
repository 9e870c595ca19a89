// Resize geometry shared by the LiTS batch kernels (lits.hip: 2-D slices, lits3d.hip: 3-D patches): TF's
// resize_bilinear / resize_nearest_neighbor with align_corners=True.  One copy, so the 2-D and 3-D pipelines cannot drift.
#pragma once
#include "common.h"

// align_corners: in = out * (in_size - 1) / (out_size - 1)
__device__ __forceinline__ float lits_ac_scale(int in_size, int out_size) {
  return out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f;
}

// the two bilinear taps of source coordinate `in` on an axis of `extent` pixels and the weight of the second
struct LitsTaps {
  int i0, i1;
  float f;
};
__device__ __forceinline__ LitsTaps lits_ac_taps(float in, int extent) {
  LitsTaps t;
  t.i0 = (int)floorf(in);
  t.i1 = min(t.i0 + 1, extent - 1);
  t.f = in - t.i0;
  return t;
}

// nearest neighbour, align_corners
__device__ __forceinline__ int lits_ac_nearest(float in, int extent) { return min((int)roundf(in), extent - 1); }

// tf resize_bilinear's lerp order: along x on both rows, then along y
__device__ __forceinline__ float lits_bilerp(float tl, float tr, float bl, float br, float lx, float ly) {
  const float top = tl + (tr - tl) * lx, bot = bl + (br - bl) * lx;
  return top + (bot - top) * ly;
}
