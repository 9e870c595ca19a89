// The crop box, the mask moments and the value of one resized pixel of the click-guided 2-D batches, shared by lits_inter.hip
// (unetk_lits_inter_batch) and lits_geodesic.hip (unetk_lits_inter_center: the geodesic guide's base field is the centre
// channel of that batch at every second pixel, bit for bit).  One copy, so the two cannot drift: the same partial blocks in
// the same order give the same m and s, and the same expression gives the same z-scored lerp.
#pragma once
#include "common.h"
#include "lits_geom.h"
#include "lits_patch.h"

namespace {

constexpr int IB_MAX_C = 7;              // image channels (odd; the channel-mask partials are 8 floats per block)

// ------------------------------------------------------------------------------------------------ crop box
struct Box2 {
  int64_t base, cz;
  int depth, y1, x1, ch, cw;
};
// DataLoader/misc.py:108-129 img_crop: the (y, x) box clamped as unetk_lits_patch3d clamps it, no clamp along z
__device__ __forceinline__ Box2 ib_box(const int32_t* __restrict__ t, const unetk_lits_inter_desc& d) {
  Box2 b;
  b.base = t[0];
  b.depth = max(t[1], 0);
  b.cz = t[2];
  b.ch = min(max(t[5], 1), d.src_h);
  b.cw = min(max(t[6], 1), d.src_w);
  b.y1 = min(max(t[3] - b.ch / 2, 0), d.src_h - b.ch);
  b.x1 = min(max(t[4] - b.cw / 2, 0), d.src_w - b.cw);
  return b;
}
// store index of slice cz + dz of the case, or -1 where it leaves the case (or the store): zero padding
__device__ __forceinline__ int64_t ib_slice(const Box2& b, int dz, const unetk_lits_inter_desc& d) {
  const int64_t zs = b.cz + dz, s = b.base + zs;
  return (zs >= 0 && zs < b.depth && s >= 0 && s < d.n_slices) ? s : -1;
}

// ------------------------------------------------------------------------------------------------ images: mask moments
// data_processing :437-440: moments over the crop's voxels with v > 0, at SOURCE resolution, all channels together.
__global__ __launch_bounds__(256) void ib_mask_stats_kernel(unetk_lits_inter_desc d, const uint16_t* __restrict__ slices,
                                                            const int32_t* __restrict__ tab, double* __restrict__ part) {
  const int n = blockIdx.y, P = gridDim.x;
  const Box2 b = ib_box(tab + (int64_t)n * TW, d);
  const int64_t plane = (int64_t)d.src_h * d.src_w;
  const int area = b.ch * b.cw;
  const int total = d.C * area;                              // < 2^31: checked by the entry point
  const float scale = (float)d.im_scale;
  double cnt = 0., sum = 0., sq = 0.;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += P * 256) {
    const int c = (int)(i / area), r = (int)(i - (int64_t)c * area);
    const int y = r / b.cw, x = r - y * b.cw;
    const int64_t s = ib_slice(b, c - d.C / 2, d);
    if (s < 0) continue;
    const float v = (float)slices[s * plane + (int64_t)(b.y1 + y) * d.src_w + b.x1 + x] / scale;
    if (v > 0.f) {
      cnt += 1.;
      sum += (double)v;
      sq += (double)v * (double)v;
    }
  }
  block_sum3(cnt, sum, sq, part + ((int64_t)n * P + blockIdx.x) * 3);
}

// ------------------------------------------------------------------------------------------------ images: one pixel
// The bilinear corners of output pixel (y, x) of the resized, un-flipped sample.
struct IbTaps {
  LitsTaps ty, tx;
  int y0, x0;
};
__device__ __forceinline__ IbTaps ib_taps(int y, int x, const Box2& b, float hs, float ws) {
  IbTaps t;
  t.ty = lits_ac_taps(y * hs, b.ch);
  t.tx = lits_ac_taps(x * ws, b.cw);
  t.y0 = min(t.ty.i0, b.ch - 1);
  t.x0 = min(t.tx.i0, b.cw - 1);
  return t;
}
// z-score of each corner, then the lerp (data_processing :442 before :468): (img - region mean) / (region sd + 1e-8).
// p: the slice at the crop box's origin.
__device__ __forceinline__ float ib_value(const uint16_t* __restrict__ p, int src_w, const IbTaps& t, float scale, float m,
                                          float den) {
  float q[4] = {(float)p[(int64_t)t.y0 * src_w + t.x0], (float)p[(int64_t)t.y0 * src_w + t.tx.i1],
                (float)p[(int64_t)t.ty.i1 * src_w + t.x0], (float)p[(int64_t)t.ty.i1 * src_w + t.tx.i1]};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float cv = q[j] / scale;
    q[j] = cv > 0.f ? (cv - m) / den : 0.f;
  }
  return lits_bilerp(q[0], q[1], q[2], q[3], t.tx.f, t.ty.f);
}

// ------------------------------------------------------------------------------------------------ host side
bool ib_valid(const unetk_lits_inter_desc* d) {
  return d && d->N > 0 && d->N <= 65535 && d->H > 0 && d->W > 0 && d->C > 0 && d->n_slices > 0 && d->src_h > 0 && d->src_w > 0 &&
         d->im_scale > 0 && d->lab_scale > 0 && d->obj_label > 0 && (int64_t)d->lab_scale * d->obj_label < ((int64_t)1 << 31) &&
         (int64_t)d->src_h * d->src_w < ((int64_t)1 << 30);
}
bool ib_supported(const unetk_lits_inter_desc* d) {
  return d->C % 2 == 1 && d->C <= IB_MAX_C && (int64_t)d->H * d->W * d->C < ((int64_t)1 << 31) &&
         (int64_t)d->C * d->src_h * d->src_w < ((int64_t)1 << 31);
}
inline int ib_blocks(const unetk_lits_inter_desc* d) { return p3d_blocks_for((int64_t)d->H * d->W * d->C); }

}  // namespace
