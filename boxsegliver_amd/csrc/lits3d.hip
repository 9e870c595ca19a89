// 3-D training patches for UNet3D, cropped and normalised on the device from the resident LiTS slice store.
//
// The reference has no LiTS 3-D pipeline; the semantics are those of its 3-D pipeline for the NF data
// (DataLoader/NF/input_pipeline_3d.py:544-604 gen_batch, :352-407 data_processing; DataLoader/misc.py:132-143 volume_crop;
// utils/image_ops.py:241 random_flip, :339-354 augment_gamma), the volumes are the cases of data/lits.SliceStore:
//   crop D x ch x cw around a centre -> z-score over the crop's non-zero voxels -> resize_bilinear(align_corners) to H x W per
//   slice -> flips -> (training) gamma with retain_stats; labels nearest.
// Everything per-sample arrives in ONE int32 table (include/unetk.h: UNETK_LITS3D_TAB_COLS); the forced-class centres are
// picked on the device (unetk_lits_pick_voxel) straight into that table, so a batch never synchronises the host.
//
// All kernels are HBM-bound passes over a few MB per sample.  The reductions (mask moments, patch moments, min / max) go
// through fp64 per-block partials in the workspace and a finalising block that walks them by index: no floating-point
// atomics, identical bits on every call.
//   workspace: double sums[N][P][3], float minmax[N][P][2] (the blocks' partials: see "block reductions"), then
//              float stat[N][8] = {m, s, mn, sd, min, range, new_mn, new_sd}
#include "common.h"
#include "lits_geom.h"
#include "lits_patch.h"      // TW, ST_*, Box3 / p3d_box, block_sum3 / block_minmax, p3d_finalize_kernel, the two gamma passes

namespace {

inline int p3d_blocks(const unetk_lits3d_desc* d) { return p3d_blocks_for((int64_t)d->D * d->H * d->W); }

// ------------------------------------------------------------------------------------------------ forced-class centre
// One block per sample; thread t owns the contiguous pixels [t L, (t + 1) L) of the slice, so a block-wide exclusive
// prefix of the per-thread counts orders the forced-class pixels row-major.
__global__ __launch_bounds__(1024) void lits_pick_voxel_kernel(const uint8_t* __restrict__ segs, int n_slices, int src_h, int src_w,
                                                              int thr, int only, int32_t* __restrict__ tab,
                                                              int32_t* __restrict__ status) {
  __shared__ int wtot[16];
  int32_t* t = tab + (int64_t)blockIdx.x * TW;
  if (t[11] == 0) return;                                    // uniform sample: keeps the (cy, cx) the host drew
  if (only != 0 && t[11] != only) return;                    // unetk_lits_pick_voxel_rows: another plane's row
  const int64_t s = (int64_t)t[0] + t[2];
  const int k = t[12];
  const bool ok = s >= 0 && s < n_slices && k >= 0;          // block-uniform
  const int hw = src_h * src_w;
  const int L = (hw + 1023) / 1024;
  const int lo = min((int)threadIdx.x * L, hw), hi = min(lo + L, hw);
  const uint8_t* p = segs + (ok ? s : 0) * (int64_t)hw;
  int cnt = 0;
  if (ok)
    for (int i = lo; i < hi; ++i) cnt += p[i] >= thr ? 1 : 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  int woff = 0, total = 0;
  for (int w = 0; w < 16; ++w) {
    if (w < wave) woff += wtot[w];
    total += wtot[w];
  }
  const int excl = woff + incl - cnt;
  if (ok && k >= excl && k < excl + cnt) {                   // exactly one thread when k < total
    int r = k - excl;
    for (int i = lo; i < hi; ++i) {
      if (p[i] >= thr) {
        if (r == 0) {
          t[3] = i / src_w;
          t[4] = i - (i / src_w) * src_w;
          break;
        }
        --r;
      }
    }
  }
  if (threadIdx.x == 0 && (!ok || k >= total)) {             // a caller bug: flagged, and a centre that is always valid
    t[3] = 0;
    t[4] = 0;
    atomicOr(status, only > 1 ? 3 : 1);                      // bit 1 (2) beside bit 0: the rank was one of another plane's rows
  }
}

// crop box: Box3, p3d_box, p3d_slice (lits_patch.h; lits3d_clicks.hip cuts the same box)

// ------------------------------------------------------------------------------------------------ pass 1: mask moments
// data_processing :354-357: moments over the crop's voxels with v > 0, at SOURCE resolution.  v = stored / im_scale is an
// integer multiple of 1 / im_scale, so the fp64 sums are exact.
__global__ __launch_bounds__(256) void p3d_mask_stats_kernel(unetk_lits3d_desc d, const uint16_t* __restrict__ slices,
                                                             const int32_t* __restrict__ tab, double* __restrict__ part) {
  const int n = blockIdx.y, P = gridDim.x;
  const Box3 b = p3d_box(tab + (int64_t)n * TW, d);
  const int64_t plane = (int64_t)d.src_h * d.src_w;
  const int area = b.ch * b.cw;
  const int total = d.D * area;                              // < 2^31: checked by the entry point
  const float scale = (float)d.im_scale;
  double cnt = 0., sum = 0., sq = 0.;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += P * 256) {
    const int z = (int)(i / area), r = (int)(i - (int64_t)z * area);
    const int y = r / b.cw, x = r - y * b.cw;
    const int64_t s = p3d_slice(b, z, d);
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

// ------------------------------------------------------------------------------------------------ pass 2: the patch
// Voxel (z, y, x) of the resized, un-flipped patch; the flips are its write address.
//
// ROT (unetk_lits_patch3d_rot): a row whose table columns 13 / 14 are not both bit-zero is turned in the
// plane about the crop's centre.  Its four taps and its label are read from the SLICE (p3d_rot_tap / p3d_rot_label), not
// from the crop box, so the corners of a turned patch show the tissue that lies there; only what leaves the slice is 0.
// The row is block-uniform (blockIdx.y); rows that are not rotated run the statements of ROT = false.  x-fastest threads
// walk a slanted line through the uint16 rows: neighbouring lanes stay within a few 64-byte segments of each other, and the
// pass is a few MB per sample either way.
__device__ __forceinline__ float p3d_rot_tap(const uint16_t* __restrict__ sl, int64_t yy, int64_t xx, int src_h, int src_w) {
  return (yy >= 0 && yy < src_h && xx >= 0 && xx < src_w) ? (float)sl[yy * src_w + xx] : 0.f;
}
__device__ __forceinline__ int p3d_rot_label(const uint8_t* __restrict__ sg, int64_t yy, int64_t xx,
                                             const unetk_lits3d_desc& d) {
  return (yy >= 0 && yy < d.src_h && xx >= 0 && xx < d.src_w) ? min((int)sg[yy * d.src_w + xx] / d.lab_scale, d.lab_max) : 0;
}
template <bool ROT>
__global__ __launch_bounds__(256) void p3d_patch_kernel(unetk_lits3d_desc d, const uint16_t* __restrict__ slices,
                                                        const uint8_t* __restrict__ segs, const int32_t* __restrict__ tab,
                                                        const float* __restrict__ stat, float* __restrict__ images,
                                                        int32_t* __restrict__ labels, double* __restrict__ part,
                                                        float* __restrict__ minmax) {
  const int n = blockIdx.y, P = gridDim.x;
  const int32_t* t = tab + (int64_t)n * TW;
  const Box3 b = p3d_box(t, d);
  const bool flr = t[7] != 0, fud = t[8] != 0, ffb = t[9] != 0;
  LitsRot rot = {false, 0.f, 0.f};
  if (ROT) rot = lits_rot_of(t);
  const float m = stat[(int64_t)n * ST_N + ST_M], den = stat[(int64_t)n * ST_N + ST_S] + 1e-8f;
  const float scale = (float)d.im_scale;
  const float hs = lits_ac_scale(b.ch, d.H), ws = lits_ac_scale(b.cw, d.W);
  const int64_t plane = (int64_t)d.src_h * d.src_w;
  const int area = d.H * d.W;
  const int total = d.D * area;                              // < 2^31: checked by the entry point
  float* img = images + (int64_t)n * total;
  int32_t* lab = labels + (int64_t)n * total;
  double cnt = 0., sum = 0., sq = 0.;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += P * 256) {
    const int z = (int)(i / area), r = (int)(i - (int64_t)z * area);
    const int y = r / d.W, x = r - y * d.W;
    const float in_y = y * hs, in_x = x * ws;
    float v = 0.f;
    int l = 0;
    const int64_t s = p3d_slice(b, z, d);
    if (ROT && rot.on) {
      const LitsRotAt at = lits_rot_coord(y, x, b.ch, b.cw, hs, ws, rot);
      if (s >= 0 && at.ok) {
        const float fy0 = floorf(at.in_y), fx0 = floorf(at.in_x);
        const int64_t yy = (int64_t)b.y1 + (int)fy0, xx = (int64_t)b.x1 + (int)fx0;
        const uint16_t* sl = slices + s * plane;
        float c[4] = {p3d_rot_tap(sl, yy, xx, d.src_h, d.src_w), p3d_rot_tap(sl, yy, xx + 1, d.src_h, d.src_w),
                      p3d_rot_tap(sl, yy + 1, xx, d.src_h, d.src_w), p3d_rot_tap(sl, yy + 1, xx + 1, d.src_h, d.src_w)};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float cv = c[j] / scale;
          c[j] = cv > 0.f ? (cv - m) / den : 0.f;
        }
        v = lits_bilerp(c[0], c[1], c[2], c[3], at.in_x - fx0, at.in_y - fy0);
        l = p3d_rot_label(segs + s * plane, (int64_t)b.y1 + (int)roundf(at.in_y), (int64_t)b.x1 + (int)roundf(at.in_x), d);
      }
    } else if (s >= 0) {
      const LitsTaps ty = lits_ac_taps(in_y, b.ch), tx = lits_ac_taps(in_x, b.cw);
      const uint16_t* p = slices + s * plane + (int64_t)b.y1 * d.src_w + b.x1;
      // z-score of each corner, then the lerp (data_processing :359 before :381): (img - region mean) / (region sd + 1e-8)
      float c[4] = {(float)p[(int64_t)ty.i0 * d.src_w + tx.i0], (float)p[(int64_t)ty.i0 * d.src_w + tx.i1],
                    (float)p[(int64_t)ty.i1 * d.src_w + tx.i0], (float)p[(int64_t)ty.i1 * d.src_w + tx.i1]};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float cv = c[j] / scale;
        c[j] = cv > 0.f ? (cv - m) / den : 0.f;
      }
      v = lits_bilerp(c[0], c[1], c[2], c[3], tx.f, ty.f);
      const int ny = lits_ac_nearest(in_y, b.ch), nx = lits_ac_nearest(in_x, b.cw);
      l = min((int)segs[s * plane + (int64_t)(b.y1 + ny) * d.src_w + b.x1 + nx] / d.lab_scale, d.lab_max);
    }
    const int zo = ffb ? d.D - 1 - z : z, yo = fud ? d.H - 1 - y : y, xo = flr ? d.W - 1 - x : x;
    const int o = (zo * d.H + yo) * d.W + xo;
    img[o] = v;
    lab[o] = l;
    cnt += 1.;
    sum += (double)v;
    sq += (double)v * (double)v;
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  if (d.training) {
    block_sum3(cnt, sum, sq, part + ((int64_t)n * P + blockIdx.x) * 3);
    block_minmax(lo, hi, minmax + ((int64_t)n * P + blockIdx.x) * 2);
  }
}

// WARP (unetk_lits_patch3d_warp): ONLY the rows whose table column 15 is not zero, launched after
// p3d_patch_kernel<true> has written every row -- the rows that are not deformed keep the bits of that compiled kernel by
// construction (lits3d_clicks.hip: click_guide3d_launch says why a branch inside one kernel does not give that).  A deformed
// row is written again, and its block partials with it, from coordinates moved by the row's B-spline lattice in front of
// the row's own map (lits_warp_coord); taps, label, z-score and flips are p3d_patch_kernel's rotated branch word for word.
// The field is the same for every slice, so a thread owns output pixels (y, x), evaluates the spline once per pixel and
// walks the slices; ZC threads share a pixel's slices when the grid has more threads than the patch has pixels.  The
// lattice (at most 2 * 19 * 19 floats) is staged in LDS: 32 reads per pixel, neighbouring lanes on the same or the next word.
__global__ __launch_bounds__(256) void p3d_warp_kernel(unetk_lits3d_desc d, const uint16_t* __restrict__ slices,
                                                       const uint8_t* __restrict__ segs, const int32_t* __restrict__ tab,
                                                       const float* __restrict__ warp, int G, const float* __restrict__ stat,
                                                       float* __restrict__ images, int32_t* __restrict__ labels,
                                                       double* __restrict__ part, float* __restrict__ minmax) {
  __shared__ float lat[2 * (LITS_WARP_MAX_G + 3) * (LITS_WARP_MAX_G + 3)];
  const int n = blockIdx.y, P = gridDim.x;
  const int32_t* t = tab + (int64_t)n * TW;
  if (t[15] == 0) return;                                    // block-uniform: p3d_patch_kernel<true> has written this row
  const int cells = (G + 3) * (G + 3);
  for (int i = threadIdx.x; i < 2 * cells; i += 256) lat[i] = warp[(int64_t)n * 2 * cells + i];
  __syncthreads();
  const Box3 b = p3d_box(t, d);
  const bool flr = t[7] != 0, fud = t[8] != 0, ffb = t[9] != 0;
  const LitsRot rot = lits_rot_of(t);
  const float m = stat[(int64_t)n * ST_N + ST_M], den = stat[(int64_t)n * ST_N + ST_S] + 1e-8f;
  const float scale = (float)d.im_scale;
  const float hs = lits_ac_scale(b.ch, d.H), ws = lits_ac_scale(b.cw, d.W);
  const int64_t plane = (int64_t)d.src_h * d.src_w;
  const int area = d.H * d.W;
  const int total = d.D * area;                              // < 2^31: checked by the entry point
  const int ZC = (int)min((int64_t)d.D, max((int64_t)1, ((int64_t)P * 256) / area));
  float* img = images + (int64_t)n * total;
  int32_t* lab = labels + (int64_t)n * total;
  double cnt = 0., sum = 0., sq = 0.;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < (int64_t)ZC * area; i += P * 256) {
    const int zc = (int)(i / area), r = (int)(i - (int64_t)zc * area);
    const int y = r / d.W, x = r - y * d.W;
    const LitsSpline sy = lits_warp_spline(y, d.H, G), sx = lits_warp_spline(x, d.W, G);
    const LitsRotAt at = lits_warp_coord(y, x, lits_warp_disp(lat, G, sy, sx), lits_warp_disp(lat + cells, G, sy, sx), b.ch, b.cw,
                                         hs, ws, rot);
    const float fy0 = at.ok ? floorf(at.in_y) : 0.f, fx0 = at.ok ? floorf(at.in_x) : 0.f;
    const int64_t yy = (int64_t)b.y1 + (int)fy0, xx = (int64_t)b.x1 + (int)fx0;
    const int64_t ly = (int64_t)b.y1 + (at.ok ? (int)roundf(at.in_y) : 0), lx = (int64_t)b.x1 + (at.ok ? (int)roundf(at.in_x) : 0);
    const float fx = at.in_x - fx0, fy = at.in_y - fy0;
    const int yo = fud ? d.H - 1 - y : y, xo = flr ? d.W - 1 - x : x;
    for (int z = zc; z < d.D; z += ZC) {
      float v = 0.f;
      int l = 0;
      const int64_t s = p3d_slice(b, z, d);
      if (s >= 0 && at.ok) {
        const uint16_t* sl = slices + s * plane;
        float c[4] = {p3d_rot_tap(sl, yy, xx, d.src_h, d.src_w), p3d_rot_tap(sl, yy, xx + 1, d.src_h, d.src_w),
                      p3d_rot_tap(sl, yy + 1, xx, d.src_h, d.src_w), p3d_rot_tap(sl, yy + 1, xx + 1, d.src_h, d.src_w)};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float cv = c[j] / scale;
          c[j] = cv > 0.f ? (cv - m) / den : 0.f;
        }
        v = lits_bilerp(c[0], c[1], c[2], c[3], fx, fy);
        l = p3d_rot_label(segs + s * plane, ly, lx, d);
      }
      const int zo = ffb ? d.D - 1 - z : z;
      const int o = (zo * d.H + yo) * d.W + xo;
      img[o] = v;
      lab[o] = l;
      cnt += 1.;
      sum += (double)v;
      sq += (double)v * (double)v;
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
  }
  if (d.training) {
    block_sum3(cnt, sum, sq, part + ((int64_t)n * P + blockIdx.x) * 3);
    block_minmax(lo, hi, minmax + ((int64_t)n * P + blockIdx.x) * 2);
  }
}

// ZSPACE (unetk_lits_patch3d_z): ONLY the rows whose crop depth cd differs from D, each launched after the
// kernel of the same pass has served every row as unetk_lits_patch3d serves it -- the rows with cd == D keep the bits of those
// compiled kernels by construction, as the rows p3d_warp_kernel leaves alone.  A resampled row's mask partials and then its
// voxels and patch partials are written again, same grid and block partition.  The mask pass walks cd slices in place of D.
__global__ __launch_bounds__(256) void p3d_mask_stats_z_kernel(unetk_lits3d_desc d, const uint16_t* __restrict__ slices,
                                                               const int32_t* __restrict__ tab, const int32_t* __restrict__ zcrop,
                                                               int zcrop_max, double* __restrict__ part) {
  const int n = blockIdx.y, P = gridDim.x;
  const int cd = p3d_zcrop(zcrop, n, zcrop_max);
  if (cd == d.D) return;                                     // block-uniform: p3d_mask_stats_kernel has served this row
  const Box3 b = p3d_box_z(tab + (int64_t)n * TW, d, cd);
  const int64_t plane = (int64_t)d.src_h * d.src_w;
  const int area = b.ch * b.cw;
  const int total = cd * area;                               // < 2^31: zcrop_max * src_h * src_w, checked by the entry point
  const float scale = (float)d.im_scale;
  double cnt = 0., sum = 0., sq = 0.;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += P * 256) {
    const int z = (int)(i / area), r = (int)(i - (int64_t)z * area);
    const int y = r / b.cw, x = r - y * b.cw;
    const int64_t s = p3d_slice(b, z, d);
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

// The patch pass of a resampled row: the 3-D crop-and-resize.  Output slice z samples crop slices i0, i1 = the align_corners taps
// of in_z = z (cd - 1) / (D - 1); each slice's in-plane value is p3d_patch_kernel's (corners z-scored on the fly, lits_bilerp),
// a slice outside the case 0, then the lerp along z; the label is the nearest crop slice's nearest pixel.  8 taps per voxel, both
// slices' taps in one thread, x-fastest threads: each slice is read in the row segments the plain kernel reads.  The second
// slice is not read where fz == 0 (v0 + 0 (v1 - v0) = v0).
__device__ __forceinline__ float p3d_plane_value(const uint16_t* __restrict__ p, int src_w, const LitsTaps& ty, const LitsTaps& tx,
                                                 float scale, float m, float den) {
  float c[4] = {(float)p[(int64_t)ty.i0 * src_w + tx.i0], (float)p[(int64_t)ty.i0 * src_w + tx.i1],
                (float)p[(int64_t)ty.i1 * src_w + tx.i0], (float)p[(int64_t)ty.i1 * src_w + tx.i1]};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float cv = c[j] / scale;
    c[j] = cv > 0.f ? (cv - m) / den : 0.f;
  }
  return lits_bilerp(c[0], c[1], c[2], c[3], tx.f, ty.f);
}
__global__ __launch_bounds__(256) void p3d_patch_z_kernel(unetk_lits3d_desc d, const uint16_t* __restrict__ slices,
                                                          const uint8_t* __restrict__ segs, const int32_t* __restrict__ tab,
                                                          const int32_t* __restrict__ zcrop, int zcrop_max,
                                                          const float* __restrict__ stat, float* __restrict__ images,
                                                          int32_t* __restrict__ labels, double* __restrict__ part,
                                                          float* __restrict__ minmax) {
  const int n = blockIdx.y, P = gridDim.x;
  const int cd = p3d_zcrop(zcrop, n, zcrop_max);
  if (cd == d.D) return;                                     // block-uniform: p3d_patch_kernel has written this row
  const int32_t* t = tab + (int64_t)n * TW;
  const Box3 b = p3d_box_z(t, d, cd);
  const bool flr = t[7] != 0, fud = t[8] != 0, ffb = t[9] != 0;
  const float m = stat[(int64_t)n * ST_N + ST_M], den = stat[(int64_t)n * ST_N + ST_S] + 1e-8f;
  const float scale = (float)d.im_scale;
  const float zs = lits_ac_scale(cd, d.D), hs = lits_ac_scale(b.ch, d.H), ws = lits_ac_scale(b.cw, d.W);
  const int64_t plane = (int64_t)d.src_h * d.src_w;
  const int64_t corner = (int64_t)b.y1 * d.src_w + b.x1;
  const int area = d.H * d.W;
  const int total = d.D * area;                              // < 2^31: checked by the entry point
  float* img = images + (int64_t)n * total;
  int32_t* lab = labels + (int64_t)n * total;
  double cnt = 0., sum = 0., sq = 0.;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += P * 256) {
    const int z = (int)(i / area), r = (int)(i - (int64_t)z * area);
    const int y = r / d.W, x = r - y * d.W;
    const float in_y = y * hs, in_x = x * ws;
    float in_z;
    {                                                        // the product rounded on its own, never fused into the fraction or the
#pragma clang fp contract(off)                               // label's rounding: slice ratios put many coordinates near a tie
      in_z = (float)z * zs;
    }
    const LitsTaps tz = lits_ac_taps(in_z, cd), ty = lits_ac_taps(in_y, b.ch), tx = lits_ac_taps(in_x, b.cw);
    const int64_t s0 = p3d_slice(b, tz.i0, d);
    float v = s0 >= 0 ? p3d_plane_value(slices + s0 * plane + corner, d.src_w, ty, tx, scale, m, den) : 0.f;
    if (tz.f != 0.f) {
      const int64_t s1 = p3d_slice(b, tz.i1, d);
      const float v1 = s1 >= 0 ? p3d_plane_value(slices + s1 * plane + corner, d.src_w, ty, tx, scale, m, den) : 0.f;
      v = v + tz.f * (v1 - v);
    }
    int l = 0;
    const int64_t sl = p3d_slice(b, lits_ac_nearest(in_z, cd), d);
    if (sl >= 0) {
      const int ny = lits_ac_nearest(in_y, b.ch), nx = lits_ac_nearest(in_x, b.cw);
      l = min((int)segs[sl * plane + (int64_t)(b.y1 + ny) * d.src_w + b.x1 + nx] / d.lab_scale, d.lab_max);
    }
    const int zo = ffb ? d.D - 1 - z : z, yo = fud ? d.H - 1 - y : y, xo = flr ? d.W - 1 - x : x;
    const int o = (zo * d.H + yo) * d.W + xo;
    img[o] = v;
    lab[o] = l;
    cnt += 1.;
    sum += (double)v;
    sq += (double)v * (double)v;
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  if (d.training) {
    block_sum3(cnt, sum, sq, part + ((int64_t)n * P + blockIdx.x) * 3);
    block_minmax(lo, hi, minmax + ((int64_t)n * P + blockIdx.x) * 2);
  }
}

// passes 3, 4 (gamma, retain_stats): lits_patch.h
bool p3d_supported(const unetk_lits3d_desc* d) {
  return (int64_t)d->D * d->H * d->W < ((int64_t)1 << 31) && (int64_t)d->D * d->src_h * d->src_w < ((int64_t)1 << 31);
}
// the _z entries: the deepest crop must index like a D-deep one, and its slice coordinates must be exact in float32
bool p3d_z_supported(const unetk_lits3d_desc* d, int zcrop_max) {
  return (int64_t)zcrop_max * d->src_h * d->src_w < ((int64_t)1 << 31) && zcrop_max < (1 << 24);
}
bool p3d_valid(const unetk_lits3d_desc* d) {
  return d && d->N > 0 && d->N <= 65535 && d->D > 0 && d->H > 0 && d->W > 0 && d->n_slices > 0 && d->src_h > 0 && d->src_w > 0 &&
         d->im_scale > 0 && d->lab_scale > 0 && d->lab_max > 0;
}

// ------------------------------------------------------------------------------------------------ evaluation: the way back
// Whole-volume evaluation in windows: the class probabilities of the windows p3d_patch_kernel cut are
// resized back from H x W to the rows' ch x cw crops and added into the case's accumulator at source resolution.  A
// gather: one thread per voxel of the rows' union box, x fastest; it walks the rows IN ORDER (the table row is
// wave-uniform: scalar loads), so every (voxel, class) has one writer and a fixed summation order -- no atomics.  A wave
// reads and writes 64 * C consecutive floats of acc; the probs taps of neighbouring threads are neighbours too.
//
// WEIGHTED (unetk_eval3d_accumulate_w): every hit is scaled by a separable window weight gz[zw] * lerp(gy) * lerp(gx), the
// in-plane factors read at the taps and fractions of the probabilities (un-flipped window), and the float volume wsum
// collects the weights in place of the hit count.  The three tables (D + H + W floats, 2 KB for a 10 x 256 x 256 window)
// are read from global memory: gz[zw] is uniform over a wave's row of voxels and the gy / gx taps of neighbouring
// threads are neighbours, so after the first wave they are hits in the CU's vector L1; staging them in LDS would cost
// every 256-voxel block D + H + W loads and a barrier to save at most five cached loads per hit.
struct EvalBox {
  int z0, y0, x0, bd, bh, bw;
};
// The weighted kernel states its fp32 arithmetic operation by operation (contraction off, fused multiply-adds spelled out),
// and states it as the compiler contracts the unweighted kernel's: the three lerps of lits_bilerp as fused multiply-adds,
// the fraction along y as the fused yw * scale - y0, the fraction along x as the difference of the rounded product.  Next
// to the weight's products the compiler would otherwise contract the same source differently (it did: 4 ulp), and
// all-ones tables would not reproduce unetk_eval3d_accumulate bit for bit (tests/test_gpu_eval3d_weighted.py pins that).
__device__ __forceinline__ float eval3d_bilerp_fma(float tl, float tr, float bl, float br, float lx, float ly) {
#pragma clang fp contract(off)
  const float top = __builtin_fmaf(tr - tl, lx, tl), bot = __builtin_fmaf(br - bl, lx, bl);
  return __builtin_fmaf(bot - top, ly, top);
}
template <int C, bool WEIGHTED>
__global__ __launch_bounds__(256) void eval3d_accumulate_kernel(unetk_lits3d_desc d, const int32_t* __restrict__ tab,
                                                                const float* __restrict__ probs, int64_t case_base,
                                                                int case_depth, EvalBox e, float* __restrict__ acc,
                                                                int32_t* __restrict__ cnt, float* __restrict__ wsum,
                                                                const float* __restrict__ gz, const float* __restrict__ gy,
                                                                const float* __restrict__ gx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t area = (int64_t)e.bh * e.bw;
  if (i >= area * e.bd) return;
  const int zb = (int)(i / area), r = (int)(i - zb * area);
  const int yb = r / e.bw;
  const int z = e.z0 + zb, y = e.y0 + yb, x = e.x0 + (r - yb * e.bw);
  const int64_t vox = ((int64_t)z * d.src_h + y) * d.src_w + x;
  float* a = acc + vox * C;
  float sum[C];
#pragma unroll
  for (int c = 0; c < C; ++c) sum[c] = a[c];
  int hits = 0;
  float wtot = 0.f;
  if constexpr (WEIGHTED) wtot = wsum[vox];
  const int win = d.D * d.H * d.W * C;                       // < 2^31: checked by the entry point
  for (int n = 0; n < d.N; ++n) {
    const int32_t* t = tab + (int64_t)n * TW;
    const Box3 b = p3d_box(t, d);
    if (b.base != case_base || b.depth != case_depth) continue;          // not this case's row: rejected on the host
    const int zw = z - b.z1, yw = y - b.y1, xw = x - b.x1;
    if (zw < 0 || zw >= d.D || yw < 0 || yw >= b.ch || xw < 0 || xw >= b.cw) continue;
    if (p3d_slice(b, zw, d) < 0) continue;                               // the window's zero slices below a shallow case
    // the inverse resize: H x W -> ch x cw, taps in the un-flipped window; the flips are the read address
    const LitsTaps ty = lits_ac_taps(yw * lits_ac_scale(d.H, b.ch), d.H), tx = lits_ac_taps(xw * lits_ac_scale(d.W, b.cw), d.W);
    const bool flr = t[7] != 0, fud = t[8] != 0, ffb = t[9] != 0;
    const int y0 = min(ty.i0, d.H - 1), x0 = min(tx.i0, d.W - 1);
    const int zr = ffb ? d.D - 1 - zw : zw;
    const int ya = fud ? d.H - 1 - y0 : y0, yb2 = fud ? d.H - 1 - ty.i1 : ty.i1;
    const int xa = flr ? d.W - 1 - x0 : x0, xb = flr ? d.W - 1 - tx.i1 : tx.i1;
    const float* p = probs + (int64_t)n * win;
    const int ra = (zr * d.H + ya) * d.W, rb = (zr * d.H + yb2) * d.W;
    const float *tl = p + (ra + xa) * C, *tr = p + (ra + xb) * C, *bl = p + (rb + xa) * C, *br = p + (rb + xb) * C;
    if constexpr (WEIGHTED) {
#pragma clang fp contract(off)
      const float sy = lits_ac_scale(d.H, b.ch), sx = lits_ac_scale(d.W, b.cw);
      const float fy = __builtin_fmaf((float)yw, sy, -(float)ty.i0), fx = (float)xw * sx - (float)tx.i0;
      // the weight: lits_bilerp's lerp form a + f (b - a), the tap itself at fraction 0
      const float wy = gy[y0] + (gy[ty.i1] - gy[y0]) * fy, wx = gx[x0] + (gx[tx.i1] - gx[x0]) * fx;
      const float w = gz[zw] * wy * wx;
#pragma unroll
      for (int c = 0; c < C; ++c) sum[c] = __builtin_fmaf(w, eval3d_bilerp_fma(tl[c], tr[c], bl[c], br[c], fx, fy), sum[c]);
      wtot += w;
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) sum[c] += lits_bilerp(tl[c], tr[c], bl[c], br[c], tx.f, ty.f);
    }
    ++hits;
  }
  if (hits == 0) return;
#pragma unroll
  for (int c = 0; c < C; ++c) a[c] = sum[c];
  if constexpr (WEIGHTED)
    wsum[vox] = wtot;
  else
    cnt[vox] += hits;
}

// ZSPACE (unetk_eval3d_accumulate_z / _wz): the way back of p3d_patch_z_kernel, a kernel of its own so that the
// instantiations above stay the compiled code they are.  A row's window holds case slices [z1, z1 + cd) (p3d_box_z); case slice
// zw of it lies at window coordinate zw (D - 1) / (cd - 1), and the hit is the lerp along z of the in-plane bilerps of window
// slices i0 and i1, each read through the row's flips.  Contraction is off for the whole kernel and every fused multiply-add is
// spelled out, in the forms of the WEIGHTED branch above -- which are the forms the compiler gives the unweighted one -- so a
// row with cd == D (in_z == zw, fz == 0, hit == the first bilerp) adds the bits either instantiation above adds.  The second
// window slice is not read where fz == 0.
template <int C, bool WEIGHTED>
__global__ __launch_bounds__(256) void eval3d_accumulate_z_kernel(unetk_lits3d_desc d, const int32_t* __restrict__ tab,
                                                                  const int32_t* __restrict__ zcrop, int zcrop_max,
                                                                  const float* __restrict__ probs, int64_t case_base,
                                                                  int case_depth, EvalBox e, float* __restrict__ acc,
                                                                  int32_t* __restrict__ cnt, float* __restrict__ wsum,
                                                                  const float* __restrict__ gz, const float* __restrict__ gy,
                                                                  const float* __restrict__ gx) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t area = (int64_t)e.bh * e.bw;
  if (i >= area * e.bd) return;
  const int zb = (int)(i / area), r = (int)(i - zb * area);
  const int yb = r / e.bw;
  const int z = e.z0 + zb, y = e.y0 + yb, x = e.x0 + (r - yb * e.bw);
  const int64_t vox = ((int64_t)z * d.src_h + y) * d.src_w + x;
  float* a = acc + vox * C;
  float sum[C];
#pragma unroll
  for (int c = 0; c < C; ++c) sum[c] = a[c];
  int hits = 0;
  float wtot = 0.f;
  if constexpr (WEIGHTED) wtot = wsum[vox];
  const int win = d.D * d.H * d.W * C;                       // < 2^31: checked by the entry point
  for (int n = 0; n < d.N; ++n) {
    const int32_t* t = tab + (int64_t)n * TW;
    const int cd = p3d_zcrop(zcrop, n, zcrop_max);           // wave-uniform, as the table row
    const Box3 b = p3d_box_z(t, d, cd);
    if (b.base != case_base || b.depth != case_depth) continue;          // not this case's row: rejected on the host
    const int zw = z - b.z1, yw = y - b.y1, xw = x - b.x1;
    if (zw < 0 || zw >= cd || yw < 0 || yw >= b.ch || xw < 0 || xw >= b.cw) continue;
    if (p3d_slice(b, zw, d) < 0) continue;                               // the window's zero slices below a shallow case
    // the inverse resize: D x H x W -> cd x ch x cw, taps in the un-flipped window; the flips are the read address
    const float sz = lits_ac_scale(d.D, cd), sy = lits_ac_scale(d.H, b.ch), sx = lits_ac_scale(d.W, b.cw);
    const LitsTaps tz = lits_ac_taps((float)zw * sz, d.D), ty = lits_ac_taps((float)yw * sy, d.H), tx = lits_ac_taps((float)xw * sx, d.W);
    const bool flr = t[7] != 0, fud = t[8] != 0, ffb = t[9] != 0;
    const int z0 = min(tz.i0, d.D - 1), y0 = min(ty.i0, d.H - 1), x0 = min(tx.i0, d.W - 1);
    const float fz = (float)zw * sz - (float)tz.i0;
    const float fy = __builtin_fmaf((float)yw, sy, -(float)ty.i0), fx = (float)xw * sx - (float)tx.i0;
    const int za = ffb ? d.D - 1 - z0 : z0, zc = ffb ? d.D - 1 - tz.i1 : tz.i1;
    const int ya = fud ? d.H - 1 - y0 : y0, yb2 = fud ? d.H - 1 - ty.i1 : ty.i1;
    const int xa = flr ? d.W - 1 - x0 : x0, xb = flr ? d.W - 1 - tx.i1 : tx.i1;
    const float* p = probs + (int64_t)n * win;
    const int ra = (za * d.H + ya) * d.W, rb = (za * d.H + yb2) * d.W;
    const float *tl = p + (ra + xa) * C, *tr = p + (ra + xb) * C, *bl = p + (rb + xa) * C, *br = p + (rb + xb) * C;
    float hit[C];
#pragma unroll
    for (int c = 0; c < C; ++c) hit[c] = eval3d_bilerp_fma(tl[c], tr[c], bl[c], br[c], fx, fy);
    if (fz != 0.f) {
      const int step = (zc - za) * d.H * d.W * C;                        // to the same taps of window slice i1
#pragma unroll
      for (int c = 0; c < C; ++c)
        hit[c] = __builtin_fmaf(eval3d_bilerp_fma(tl[step + c], tr[step + c], bl[step + c], br[step + c], fx, fy) - hit[c], fz, hit[c]);
    }
    if constexpr (WEIGHTED) {
      // the weight: lits_bilerp's lerp form a + f (b - a) on every axis, the tap itself at fraction 0
      const float wz = gz[z0] + (gz[tz.i1] - gz[z0]) * fz;
      const float wy = gy[y0] + (gy[ty.i1] - gy[y0]) * fy, wx = gx[x0] + (gx[tx.i1] - gx[x0]) * fx;
      const float w = wz * wy * wx;
#pragma unroll
      for (int c = 0; c < C; ++c) sum[c] = __builtin_fmaf(w, hit[c], sum[c]);
      wtot += w;
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) sum[c] = sum[c] + hit[c];
    }
    ++hits;
  }
  if (hits == 0) return;
#pragma unroll
  for (int c = 0; c < C; ++c) a[c] = sum[c];
  if constexpr (WEIGHTED)
    wsum[vox] = wtot;
  else
    cnt[vox] += hits;
}

// The end of a case (unetk_eval3d_finish): one thread per voxel of the volume.  A voxel is covered when its weight (wsum or
// cnt) is positive; a covered voxel of the box `e` gets the argmax of its C sums, strict > so that the lowest index wins ties
// (as head_predict_kernel, csrc/head.hip), every other voxel class 0.  Voxels of `e` without cover are counted: one integer
// atomic per wave that has any (the idiom of lc_flatten_kernel, csrc/evalvol.hip) -- integer adds commute, the count is
// reproducible.
__global__ __launch_bounds__(256) void eval3d_finish_kernel(const float* __restrict__ acc, int C, int64_t nvox, int src_h,
                                                            int src_w, const float* __restrict__ wsum,
                                                            const int32_t* __restrict__ cnt, EvalBox e,
                                                            uint8_t* __restrict__ pred, int32_t* __restrict__ uncovered) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool missing = false;
  if (i < nvox) {
    const int64_t plane = (int64_t)src_h * src_w;
    const int z = (int)(i / plane), r = (int)(i - z * plane);
    const int y = r / src_w, x = r - y * src_w;
    const bool inside = z >= e.z0 && z < e.z0 + e.bd && y >= e.y0 && y < e.y0 + e.bh && x >= e.x0 && x < e.x0 + e.bw;
    const bool covered = wsum ? wsum[i] > 0.f : cnt[i] > 0;
    int bi = 0;
    if (inside && covered) {
      const float* a = acc + i * C;
      float best = a[0];
      for (int k = 1; k < C; ++k) {
        const float v = a[k];
        if (v > best) {
          best = v;
          bi = k;
        }
      }
    }
    missing = inside && !covered;
    pred[i] = (uint8_t)bi;
  }
  const unsigned long long any = __ballot(missing);
  if (missing && (int)__lane_id() == __ffsll((long long)any) - 1) atomicAdd(uncovered, __popcll(any));
}

}  // namespace

// Both accumulate entry points: cnt for the plain one, wsum and the three tables for the weighted one.
// zspace: the _z / _wz entries, which take the rows' crop depths (zcrop, zcrop_max) and launch eval3d_accumulate_z_kernel.
static int eval3d_accumulate(const unetk_lits3d_desc* d, const int32_t* sample_tab, const float* probs, int C, int64_t case_base,
                             int case_depth, const int32_t box[6], float* acc, int32_t* cnt, float* wsum, const float* gz,
                             const float* gy, const float* gx, void* stream, bool zspace = false, const int32_t* zcrop = nullptr,
                             int zcrop_max = 0) {
  const bool weighted = cnt == nullptr;
  UNETK_REQUIRE(!zspace || (zcrop && (((uintptr_t)zcrop) & 3u) == 0 && zcrop_max >= 1));
  UNETK_REQUIRE(p3d_valid(d) && sample_tab && probs && box && acc && C >= 1 && C <= 8);
  UNETK_REQUIRE(((((uintptr_t)sample_tab) | ((uintptr_t)probs) | ((uintptr_t)acc) | ((uintptr_t)cnt)) & 3u) == 0);
  UNETK_REQUIRE(!weighted || (wsum && gz && gy && gx &&
                              ((((uintptr_t)wsum) | ((uintptr_t)gz) | ((uintptr_t)gy) | ((uintptr_t)gx)) & 3u) == 0));
  UNETK_REQUIRE(case_base >= 0 && case_depth > 0 && case_base + case_depth <= d->n_slices);
  UNETK_REQUIRE(0 <= box[0] && box[0] < box[1] && box[1] <= case_depth && 0 <= box[2] && box[2] < box[3] && box[3] <= d->src_h &&
                0 <= box[4] && box[4] < box[5] && box[5] <= d->src_w);
  if (!p3d_supported(d) || (int64_t)d->D * d->H * d->W * C >= ((int64_t)1 << 31)) return UNETK_E_UNSUPPORTED;
  if (zspace && !p3d_z_supported(d, zcrop_max)) return UNETK_E_UNSUPPORTED;
  const EvalBox e = {box[0], box[2], box[4], box[1] - box[0], box[3] - box[2], box[5] - box[4]};
  const int64_t blocks = ((int64_t)e.bd * e.bh * e.bw + 255) / 256;
  if (blocks >= ((int64_t)1 << 31)) return UNETK_E_UNSUPPORTED;
  const dim3 grid((unsigned)blocks);
  hipStream_t st = (hipStream_t)stream;
#define EVAL3D_CASE_Z(c)                                                                                                    \
  case c:                                                                                                                   \
    if (weighted)                                                                                                           \
      UNETK_LAUNCH((eval3d_accumulate_z_kernel<c, true>), grid, dim3(256), 0, st, *d, sample_tab, zcrop, zcrop_max, probs,   \
                   case_base, case_depth, e, acc, cnt, wsum, gz, gy, gx);                                                    \
    else                                                                                                                    \
      UNETK_LAUNCH((eval3d_accumulate_z_kernel<c, false>), grid, dim3(256), 0, st, *d, sample_tab, zcrop, zcrop_max, probs,  \
                   case_base, case_depth, e, acc, cnt, wsum, gz, gy, gx);                                                    \
    break;
#define EVAL3D_CASE(c)                                                                                                      \
  case c:                                                                                                                   \
    if (weighted)                                                                                                           \
      UNETK_LAUNCH((eval3d_accumulate_kernel<c, true>), grid, dim3(256), 0, st, *d, sample_tab, probs, case_base, case_depth, e, \
                   acc, cnt, wsum, gz, gy, gx);                                                                             \
    else                                                                                                                    \
      UNETK_LAUNCH((eval3d_accumulate_kernel<c, false>), grid, dim3(256), 0, st, *d, sample_tab, probs, case_base, case_depth, e, \
                   acc, cnt, wsum, gz, gy, gx);                                                                             \
    break;
  if (zspace) {
    switch (C) {
      EVAL3D_CASE_Z(1) EVAL3D_CASE_Z(2) EVAL3D_CASE_Z(3) EVAL3D_CASE_Z(4) EVAL3D_CASE_Z(5) EVAL3D_CASE_Z(6) EVAL3D_CASE_Z(7) EVAL3D_CASE_Z(8)
    }
  } else {
    switch (C) {
      EVAL3D_CASE(1) EVAL3D_CASE(2) EVAL3D_CASE(3) EVAL3D_CASE(4) EVAL3D_CASE(5) EVAL3D_CASE(6) EVAL3D_CASE(7) EVAL3D_CASE(8)
    }
  }
#undef EVAL3D_CASE
#undef EVAL3D_CASE_Z
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_eval3d_accumulate(const unetk_lits3d_desc* d, const int32_t* sample_tab, const float* probs, int C,
                                       int64_t case_base, int case_depth, const int32_t box[6], float* acc, int32_t* cnt,
                                       void* stream) {
  UNETK_REQUIRE(cnt);
  return eval3d_accumulate(d, sample_tab, probs, C, case_base, case_depth, box, acc, cnt, nullptr, nullptr, nullptr, nullptr,
                           stream);
}

extern "C" int unetk_eval3d_accumulate_w(const unetk_lits3d_desc* d, const int32_t* sample_tab, const float* probs, int C,
                                         int64_t case_base, int case_depth, const int32_t box[6], const float* gz,
                                         const float* gy, const float* gx, float* acc, float* wsum, void* stream) {
  UNETK_REQUIRE(wsum && gz && gy && gx);
  return eval3d_accumulate(d, sample_tab, probs, C, case_base, case_depth, box, acc, nullptr, wsum, gz, gy, gx, stream);
}

extern "C" int unetk_eval3d_accumulate_z(const unetk_lits3d_desc* d, const int32_t* sample_tab, const int32_t* zcrop, int zcrop_max,
                                         const float* probs, int C, int64_t case_base, int case_depth, const int32_t box[6],
                                         float* acc, int32_t* cnt, void* stream) {
  UNETK_REQUIRE(cnt);
  return eval3d_accumulate(d, sample_tab, probs, C, case_base, case_depth, box, acc, cnt, nullptr, nullptr, nullptr, nullptr,
                           stream, true, zcrop, zcrop_max);
}

extern "C" int unetk_eval3d_accumulate_wz(const unetk_lits3d_desc* d, const int32_t* sample_tab, const int32_t* zcrop,
                                          int zcrop_max, const float* probs, int C, int64_t case_base, int case_depth,
                                          const int32_t box[6], const float* gz, const float* gy, const float* gx, float* acc,
                                          float* wsum, void* stream) {
  UNETK_REQUIRE(wsum && gz && gy && gx);
  return eval3d_accumulate(d, sample_tab, probs, C, case_base, case_depth, box, acc, nullptr, wsum, gz, gy, gx, stream, true,
                           zcrop, zcrop_max);
}

extern "C" int unetk_eval3d_finish(const float* acc, int C, int depth, int src_h, int src_w, const float* wsum,
                                   const int32_t* cnt, const int32_t box[6], uint8_t* pred, int32_t* uncovered, void* stream) {
  UNETK_REQUIRE(acc && box && pred && uncovered && C >= 1 && C <= 8 && depth > 0 && src_h > 0 && src_w > 0);
  UNETK_REQUIRE((wsum != nullptr) != (cnt != nullptr));                   // exactly one kind of weight
  UNETK_REQUIRE(((((uintptr_t)acc) | ((uintptr_t)wsum) | ((uintptr_t)cnt) | ((uintptr_t)uncovered)) & 3u) == 0);
  UNETK_REQUIRE(0 <= box[0] && box[0] < box[1] && box[1] <= depth && 0 <= box[2] && box[2] < box[3] && box[3] <= src_h &&
                0 <= box[4] && box[4] < box[5] && box[5] <= src_w);
  const int64_t nvox = (int64_t)depth * src_h * src_w;
  if (nvox >= ((int64_t)1 << 31)) return UNETK_E_UNSUPPORTED;             // the limit of unetk_eval3d_accumulate's volume
  const EvalBox e = {box[0], box[2], box[4], box[1] - box[0], box[3] - box[2], box[5] - box[4]};
  UNETK_LAUNCH(eval3d_finish_kernel, dim3((unsigned)((nvox + 255) / 256)), dim3(256), 0, (hipStream_t)stream, acc, C, nvox, src_h,
               src_w, wsum, cnt, e, pred, uncovered);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_lits_pick_voxel(const uint8_t* seg_slices, int n_slices, int src_h, int src_w, int lab_scale, int fg_label,
                                     int32_t* sample_tab, int N, int32_t* status, void* stream) {
  UNETK_REQUIRE(seg_slices && sample_tab && status && n_slices > 0 && src_h > 0 && src_w > 0 && N > 0 && lab_scale > 0 && fg_label > 0);
  UNETK_REQUIRE((int64_t)src_h * src_w < ((int64_t)1 << 30) && (int64_t)lab_scale * fg_label < ((int64_t)1 << 31));
  UNETK_REQUIRE(((((uintptr_t)sample_tab) | ((uintptr_t)status)) & 3u) == 0);
  UNETK_LAUNCH(lits_pick_voxel_kernel, dim3(N), dim3(1024), 0, (hipStream_t)stream, seg_slices, n_slices, src_h, src_w,
               lab_scale * fg_label, 0, sample_tab, status);   // seg / lab_scale >= fg  <=>  seg >= fg * lab_scale
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_lits_pick_voxel_rows(const uint8_t* seg_slices, int n_slices, int src_h, int src_w, int lab_scale, int fg_label,
                                          int32_t* sample_tab, int N, int32_t* status, int forced_value, void* stream) {
  UNETK_REQUIRE(seg_slices && sample_tab && status && n_slices > 0 && src_h > 0 && src_w > 0 && N > 0 && lab_scale > 0 && fg_label > 0);
  UNETK_REQUIRE((int64_t)src_h * src_w < ((int64_t)1 << 30) && (int64_t)lab_scale * fg_label < ((int64_t)1 << 31));
  UNETK_REQUIRE(((((uintptr_t)sample_tab) | ((uintptr_t)status)) & 3u) == 0 && forced_value > 0);
  UNETK_LAUNCH(lits_pick_voxel_kernel, dim3(N), dim3(1024), 0, (hipStream_t)stream, seg_slices, n_slices, src_h, src_w,
               lab_scale * fg_label, forced_value, sample_tab, status);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" size_t unetk_lits_patch3d_ws_bytes(const unetk_lits3d_desc* d) {
  if (!p3d_valid(d) || !p3d_supported(d)) return 0;
  return (size_t)d->N * p3d_blocks(d) * (3 * sizeof(double) + 2 * sizeof(float)) + (size_t)d->N * ST_N * sizeof(float);
}

// The patch entry points: the same passes, the patch pass reading the table's rotation columns or not; with a lattice
// (unetk_lits_patch3d_warp: ROT, warp != nullptr) the deformed rows are then written again by p3d_warp_kernel.  zspace
// (unetk_lits_patch3d_z): the rows whose crop depth is not D get their mask partials and then their voxels written again, by
// p3d_mask_stats_z_kernel and p3d_patch_z_kernel.
template <bool ROT>
static int lits_patch3d(const unetk_lits3d_desc* d, const uint16_t* slices, const uint8_t* seg_slices,
                        const int32_t* sample_tab, float* images, int32_t* labels, void* ws, size_t ws_bytes, void* stream,
                        const float* warp = nullptr, int G = 0, bool zspace = false, const int32_t* zcrop = nullptr,
                        int zcrop_max = 0) {
  UNETK_REQUIRE(p3d_valid(d) && slices && seg_slices && sample_tab && images && labels && ws);
  UNETK_REQUIRE(!zspace || (zcrop && (((uintptr_t)zcrop) & 3u) == 0 && zcrop_max >= 1));
  UNETK_REQUIRE((((uintptr_t)slices) & 1u) == 0 && ((((uintptr_t)sample_tab) | ((uintptr_t)images) | ((uintptr_t)labels)) & 3u) == 0);
  UNETK_REQUIRE(unetk_aligned16(ws));
  if (!p3d_supported(d) || (zspace && !p3d_z_supported(d, zcrop_max))) return UNETK_E_UNSUPPORTED;
  if (ws_bytes < unetk_lits_patch3d_ws_bytes(d)) return UNETK_E_WORKSPACE;
  const int P = p3d_blocks(d);
  double* part = static_cast<double*>(ws);
  float* minmax = reinterpret_cast<float*>(part + (size_t)d->N * P * 3);
  float* stat = minmax + (size_t)d->N * P * 2;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(P, d->N), fin(d->N);
  UNETK_LAUNCH(p3d_mask_stats_kernel, grid, dim3(256), 0, st, *d, slices, sample_tab, part);
  if (zspace)
    UNETK_LAUNCH(p3d_mask_stats_z_kernel, grid, dim3(256), 0, st, *d, slices, sample_tab, zcrop, zcrop_max, part);
  UNETK_LAUNCH(p3d_finalize_kernel, fin, dim3(64), 0, st, 0, P, (const double*)part, (const float*)minmax, stat);
  UNETK_LAUNCH(p3d_patch_kernel<ROT>, grid, dim3(256), 0, st, *d, slices, seg_slices, sample_tab, (const float*)stat, images, labels, part, minmax);
  if (zspace)
    UNETK_LAUNCH(p3d_patch_z_kernel, grid, dim3(256), 0, st, *d, slices, seg_slices, sample_tab, zcrop, zcrop_max, (const float*)stat, images, labels, part, minmax);
  if (warp)
    UNETK_LAUNCH(p3d_warp_kernel, grid, dim3(256), 0, st, *d, slices, seg_slices, sample_tab, warp, G, (const float*)stat, images, labels, part, minmax);
  if (d->training) {
    const int total = d->D * d->H * d->W;                      // < 2^31: p3d_supported
    UNETK_LAUNCH(p3d_finalize_kernel, fin, dim3(64), 0, st, 1, P, (const double*)part, (const float*)minmax, stat);
    UNETK_LAUNCH(p3d_gamma_kernel, grid, dim3(256), 0, st, total, sample_tab, (const float*)stat, images, part);
    UNETK_LAUNCH(p3d_finalize_kernel, fin, dim3(64), 0, st, 2, P, (const double*)part, (const float*)minmax, stat);
    UNETK_LAUNCH(p3d_retain_kernel, grid, dim3(256), 0, st, total, (const float*)stat, images);
  }
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_lits_patch3d(const unetk_lits3d_desc* d, const uint16_t* slices, const uint8_t* seg_slices,
                                  const int32_t* sample_tab, float* images, int32_t* labels, void* ws, size_t ws_bytes,
                                  void* stream) {
  return lits_patch3d<false>(d, slices, seg_slices, sample_tab, images, labels, ws, ws_bytes, stream);
}

extern "C" int unetk_lits_patch3d_z(const unetk_lits3d_desc* d, const uint16_t* slices, const uint8_t* seg_slices,
                                    const int32_t* sample_tab, const int32_t* zcrop, int zcrop_max, float* images,
                                    int32_t* labels, void* ws, size_t ws_bytes, void* stream) {
  return lits_patch3d<false>(d, slices, seg_slices, sample_tab, images, labels, ws, ws_bytes, stream, nullptr, 0, true, zcrop,
                             zcrop_max);
}

extern "C" int unetk_lits_patch3d_rot(const unetk_lits3d_desc* d, const uint16_t* slices, const uint8_t* seg_slices,
                                      const int32_t* sample_tab, float* images, int32_t* labels, void* ws, size_t ws_bytes,
                                      void* stream) {
  return lits_patch3d<true>(d, slices, seg_slices, sample_tab, images, labels, ws, ws_bytes, stream);
}

extern "C" int unetk_lits_patch3d_warp(const unetk_lits3d_desc* d, const uint16_t* slices, const uint8_t* seg_slices,
                                       const int32_t* sample_tab, const float* warp, int G, float* images, int32_t* labels,
                                       void* ws, size_t ws_bytes, void* stream) {
  UNETK_REQUIRE(warp && (((uintptr_t)warp) & 3u) == 0 && G >= 1 && G <= LITS_WARP_MAX_G);
  return lits_patch3d<true>(d, slices, seg_slices, sample_tab, images, labels, ws, ws_bytes, stream, warp, G);
}
