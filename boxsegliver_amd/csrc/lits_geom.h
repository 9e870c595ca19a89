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

// Elastic deformation of the 3-D patches (unetk_lits_patch3d_warp, unetk_click_guide3d_warp).  Column 15 of a
// LiTS 3-D table row: 0 = the row is not deformed, anything else = it is, by its lattice of control displacements
// lat f32 [2][G + 3][G + 3] (0 = dy, 1 = dx, in pixels of the output patch), a uniform cubic B-spline over G x G cells.
constexpr int LITS_WARP_MAX_G = 16;
// cell and the four B-spline weights of output index `o` on an axis of `extent` pixels; the last pixel is cell G - 1 at f = 1
struct LitsSpline {
  int i;
  float w[4];
};
__device__ __forceinline__ LitsSpline lits_warp_spline(int o, int extent, int G) {
#pragma clang fp contract(off)
  const float g = extent > 1 ? (float)G / (float)(extent - 1) : 0.f;
  const float t = (float)o * g;
  LitsSpline s;
  s.i = min((int)floorf(t), G - 1);
  const float f = t - (float)s.i, r = 1.f - f, k6 = 1.f / 6.f;
  s.w[0] = ((r * r) * r) * k6;
  s.w[1] = ((((3.f * f) - 6.f) * f) * f + 4.f) * k6;
  s.w[2] = (((((-3.f * f) + 3.f) * f + 3.f) * f) + 1.f) * k6;
  s.w[3] = ((f * f) * f) * k6;
  return s;
}
// one component of the displacement: sum_a wy[a] * (sum_b wx[b] * lat[i + a][j + b]), both sums left to right from term 0
__device__ __forceinline__ float lits_warp_disp(const float* lat, int G, const LitsSpline& sy, const LitsSpline& sx) {
#pragma clang fp contract(off)
  const int pitch = G + 3;
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float* row = lat + (sy.i + a) * pitch + sx.i;
    float in = sx.w[0] * row[0];
#pragma unroll
    for (int b = 1; b < 4; ++b) in = in + sx.w[b] * row[b];
    acc = a == 0 ? sy.w[0] * in : acc + sy.w[a] * in;
  }
  return acc;
}
// Where output pixel (y, x) lands in its ch x cw crop: the deformation acts in the OUTPUT frame, (y', x') = (y + dy, x + dx),
// and the row's own map follows -- the align_corners scale, or with a rotation the sums of lits_rot_coord.  (dy, dx): what
// lits_warp_disp gave for the two components.  Contraction off and `ok` as lits_rot_coord.
__device__ __forceinline__ LitsRotAt lits_warp_coord(int y, int x, float dy, float dx, int ch, int cw, float hs, float ws,
                                                     const LitsRot& r) {
#pragma clang fp contract(off)
  const float yp = (float)y + dy, xp = (float)x + dx;
  LitsRotAt a;
  if (r.on) {
    const float cy0 = 0.5f * (float)(ch - 1), cx0 = 0.5f * (float)(cw - 1);
    const float u = yp * hs - cy0, v = xp * ws - cx0;
    a.in_y = cy0 + (r.c * u - r.s * v);
    a.in_x = cx0 + (r.s * u + r.c * v);
  } else {
    a.in_y = yp * hs;
    a.in_x = xp * ws;
  }
  a.ok = fabsf(a.in_y) < 16777216.f && fabsf(a.in_x) < 16777216.f;        // false for NaN and infinities
  return a;
}

// tf resize_bilinear's lerp order: along x on both rows, then along y
__device__ __forceinline__ float lits_bilerp(float tl, float tr, float bl, float br, float lx, float ly) {
  const float top = tl + (tr - tl) * lx, bot = bl + (br - bl) * lx;
  return top + (bot - top) * ly;
}
