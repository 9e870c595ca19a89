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

// In-plane rotation of the 3-D patches (unetk_lits_patch3d_rot, unetk_click_guide3d_rot).  Columns 13 / 14 of
// a LiTS 3-D table row carry sin and cos as float bits; both bit-zero = the row is not rotated.
struct LitsRot {
  bool on;
  float s, c;
};
__device__ __forceinline__ LitsRot lits_rot_of(const int32_t* __restrict__ t) {
  LitsRot r;
  r.on = (t[13] | t[14]) != 0;
  r.s = __int_as_float(t[13]);
  r.c = __int_as_float(t[14]);
  return r;
}
// Where output pixel (y, x) of an H x W patch lands in its ch x cw crop, turned about the crop's centre.  Contraction is off:
// every operation rounds on its own, so that a float32 restatement forms the same bits (labels round these coordinates, and
// at 45 degrees a tenth of them sit within 1e-3 of a tie).  ok: both finite and below 2^24 in magnitude, so that floorf and
// roundf convert to int exactly; anything else counts as outside the slice.
struct LitsRotAt {
  float in_y, in_x;
  bool ok;
};
__device__ __forceinline__ LitsRotAt lits_rot_coord(int y, int x, int ch, int cw, float hs, float ws, const LitsRot& r) {
#pragma clang fp contract(off)
  const float cy0 = 0.5f * (float)(ch - 1), cx0 = 0.5f * (float)(cw - 1);
  const float u = (float)y * hs - cy0, v = (float)x * ws - cx0;
  LitsRotAt a;
  a.in_y = cy0 + (r.c * u - r.s * v);
  a.in_x = cx0 + (r.s * u + r.c * v);
  a.ok = fabsf(a.in_y) < 16777216.f && fabsf(a.in_x) < 16777216.f;        // false for NaN and infinities
  return a;
}

// tf resize_bilinear's lerp order: along x on both rows, then along y
__device__ __forceinline__ float lits_bilerp(float tl, float tr, float bl, float br, float lx, float ly) {
  const float top = tl + (tr - tl) * lx, bot = bl + (br - bl) * lx;
  return top + (bot - top) * ly;
}
