// The slice prior of click-guided UNet3D: a second image channel that tells the net what the object looks
// like on the slice z0 of the first foreground click -- the reference's --use_cascade without --use_2d
// (DataLoader/NF/input_pipeline_3d.py:505-533 gen_kernel, entry/main_eval_3d.py:348-369).  include/unetk.h has the full statement.
//
// The reference runs a 3-D Euclidean distance transform whose seeds all lie in slice z0, so
//   dist(z, y, x)^2 = (z - z0)^2 + D2(y, x),     D2 = the exact squared 2-D EDT of the boundary of slice z0, an integer field.
// The field is therefore ONE slice of int32 per row, in two separable passes:
//   sp_rows_kernel   block per (box row, table row): the object mask and its inner boundary (a foreground pixel with a background
//                    4-neighbour INSIDE the box) as one bit per pixel in LDS, 64 pixels per ballot; every pixel then finds the
//                    nearest set bit of its row (edt_int.h) -> g(y, x)^2, or IEDT_NONE in a row without a boundary pixel.
//                    Binary mode writes the mask itself and stops here.
//   sp_cols_kernel   block per 64 columns x 16 rows of the box: D2(y, x) = min over y' of (y - y')^2 + g(y', x)^2 by brute force
//                    (edt_int.h).  A box without a boundary pixel has IEDT_NONE everywhere, which the minimum shows: such a
//                    pixel gets the sentinel -1.
//   sp_render_kernel thread per output voxel: channel 0 copies the one-channel patch, channel 1 evaluates
//                    exp(-sqrt(dz^2 + D2) / 25) at the four in-plane bilinear corners and lerps (create, then resize, as
//                    click_guide3d_kernel); the three flips are the write address.
// Integer arithmetic up to the render, no atomics: two calls give identical bits.
#include "common.h"
#include "edt_int.h"
#include "lits_geom.h"
#include "lits_patch.h"      // TW, Box3, p3d_box, p3d_slice

namespace {

constexpr int SP_MAX_EXTENT = IEDT_MAX_BITS;   // src_h, src_w: a box row is one bit row of sp_rows_kernel
static_assert(iedt_fits(1, SP_MAX_EXTENT), "sp_cols_kernel overflows int32");
static_assert(2 * (int64_t)(SP_MAX_EXTENT - 1) * (SP_MAX_EXTENT - 1) < IEDT_NONE, "a real D2 reaches the sentinel");
constexpr int MAXK = UNETK_LITS_MAX_CLICKS;

// The box a row's field covers and the store slice it reads: the row's crop box with z0 relative to it, or (whole) the whole
// slice with z0 counted from the case's first slice.  slice < 0: there is no such slice, the mask is all background.
struct PriorBox {
  int y1, x1, bh, bw;
  int64_t slice;
};
__device__ __forceinline__ PriorBox sp_box(const int32_t* __restrict__ t, const unetk_lits3d_clicks_desc& d, int whole, int z0) {
  const Box3 b = p3d_box(t, d);
  PriorBox p;
  if (whole) {
    p.y1 = p.x1 = 0;
    p.bh = d.src_h;
    p.bw = d.src_w;
    const int64_t s = b.base + z0;
    p.slice = (z0 >= 0 && z0 < b.depth && s >= 0 && s < d.n_slices) ? s : -1;
  } else {
    p.y1 = b.y1;
    p.x1 = b.x1;
    p.bh = b.ch;
    p.bw = b.cw;
    p.slice = (z0 >= 0 && z0 < d.D) ? p3d_slice(b, z0, d) : -1;
  }
  return p;
}
// the slice of the first foreground click, or -1 without one.  K == 0: lists per row, pts [N][2][MAXK][3] and cnt [N][2];
// else ONE pair of lists, pts [2][K][3] and cnt [2]
__device__ __forceinline__ int sp_z0(const int32_t* __restrict__ pts, const int32_t* __restrict__ cnt, int K, int n) {
  const bool has = cnt[K ? 0 : (int64_t)n * 2] > 0;
  return has ? pts[K ? 0 : (int64_t)n * 2 * MAXK * 3] : -1;
}

// ------------------------------------------------------------------------------------------------ rows
__global__ __launch_bounds__(256) void sp_rows_kernel(unetk_lits3d_clicks_desc d, const uint8_t* __restrict__ segs,
                                                      const int32_t* __restrict__ tab, const int32_t* __restrict__ pts,
                                                      const int32_t* __restrict__ cnt, int K, int whole, int binary,
                                                      int32_t* __restrict__ out, int32_t* __restrict__ z0_out) {
  __shared__ unsigned long long bits[SP_MAX_EXTENT / 64];
  const int n = blockIdx.y, y = blockIdx.x;
  const int z0 = sp_z0(pts, cnt, K, n);
  const PriorBox p = sp_box(tab + (int64_t)n * TW, d, whole, z0);
  if (y == 0 && threadIdx.x == 0) z0_out[n] = z0;
  if (y >= p.bh) return;                                     // block-uniform
  const int64_t plane = (int64_t)d.src_h * d.src_w;
  const int thr = d.obj_label * d.lab_scale, bw = p.bw, bh = p.bh;
  const bool live = p.slice >= 0;
  // the box's row y, and its neighbours where they lie inside the box (else the row itself: a neighbour that changes nothing)
  const uint8_t* row = segs + (live ? p.slice : 0) * plane + (int64_t)(p.y1 + y) * d.src_w + p.x1;
  const uint8_t* up = y > 0 ? row - d.src_w : row;
  const uint8_t* dn = y + 1 < bh ? row + d.src_w : row;
  int32_t* o = out + (int64_t)n * plane + (int64_t)y * bw;
  const int lane = threadIdx.x & 63;
  for (int x0 = 0; x0 < bw; x0 += 256) {                     // block-uniform trip count: the ballots see whole waves
    const int x = x0 + threadIdx.x;
    bool m = false, edge = false;
    if (live && x < bw) {
      m = row[x] >= thr;
      const bool all = up[x] >= thr && dn[x] >= thr && row[max(x - 1, 0)] >= thr && row[min(x + 1, bw - 1)] >= thr;
      edge = m && !all;
    }
    if (binary) {
      if (x < bw) o[x] = m ? 1 : 0;
    } else {
      const unsigned long long w = __ballot(edge);
      if (lane == 0) bits[x >> 6] = w;
    }
  }
  if (binary) return;
  __syncthreads();
  for (int x = threadIdx.x; x < bw; x += 256) {
    const int g = iedt_nearest_bit(bits, (bw + 63) >> 6, x);
    o[x] = g < 0 ? IEDT_NONE : g * g;
  }
}

// ------------------------------------------------------------------------------------------------ columns
__global__ __launch_bounds__(256) void sp_cols_kernel(unetk_lits3d_clicks_desc d, const int32_t* __restrict__ tab,
                                                      const int32_t* __restrict__ z0s, int whole,
                                                      const int32_t* __restrict__ gsq, int32_t* __restrict__ field) {
  __shared__ int stage[IEDT_STAGE][64];
  const int n = blockIdx.z;
  const PriorBox p = sp_box(tab + (int64_t)n * TW, d, whole, z0s[n]);
  const int xb = blockIdx.x * 64, yb = blockIdx.y * IEDT_T;
  if (xb >= p.bw || yb >= p.bh) return;                      // block-uniform
  const int bw = p.bw, bh = p.bh;
  const int64_t plane = (int64_t)d.src_h * d.src_w;
  const int x = xb + (threadIdx.x & 63), y0 = yb + (threadIdx.x >> 6) * 4;   // the thread's outputs: rows y0 .. y0 + 3 of column x
  int best[4];
  iedt_axis_min(stage, gsq + (int64_t)n * plane + x, x < bw, bw, bh, y0, 1, best);
  if (x >= bw) return;
  int32_t* f = field + (int64_t)n * plane;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (y0 + k < bh) f[(int64_t)(y0 + k) * bw + x] = best[k] < IEDT_NONE ? best[k] : -1;
}

// ------------------------------------------------------------------------------------------------ render
// the prior at one pixel of the field's box and dz slices from z0
__device__ __forceinline__ float sp_at(const int32_t* __restrict__ f, int pitch, int i, int j, int dz, int binary) {
  const int v = f[(int64_t)i * pitch + j];
  if (binary) return dz == 0 && v != 0 ? 1.f : 0.f;
  if (v < 0) return 0.f;                                     // the sentinel: no click, or a slice without a boundary
  return expf(-sqrtf((float)((int64_t)dz * dz + v)) / 25.f);
}
// SHARED: ONE field over the whole slice [src_h, src_w] and ONE z0, both in case coordinates, for every row; else a field per
// row over its crop box (pitch cw) and z0 [N] relative to it
template <bool SHARED>
__global__ __launch_bounds__(256) void sp_render_kernel(unetk_lits3d_clicks_desc d, const int32_t* __restrict__ tab,
                                                        const float* __restrict__ img1, const int32_t* __restrict__ field,
                                                        const int32_t* __restrict__ z0s, int binary, float* __restrict__ img2) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int area = d.H * d.W, vol = d.D * area;              // < 2^31: checked by the entry point
  if (i >= (int64_t)d.N * vol) return;
  const int n = (int)(i / vol), r = (int)(i - (int64_t)n * vol);
  const int z = r / area, q = r - z * area;
  const int y = q / d.W, x = q - y * d.W;
  const int32_t* t = tab + (int64_t)n * TW;
  const Box3 b = p3d_box(t, d);
  // resize_bilinear(align_corners) from ch x cw: the taps and fractions of click_guide3d_kernel, every operation rounded on
  // its own
  const float in_y = (float)y * lits_ac_scale(b.ch, d.H), in_x = (float)x * lits_ac_scale(b.cw, d.W);
  const float fy0 = floorf(in_y), fx0 = floorf(in_x);
  const int i0 = min((int)fy0, b.ch - 1), j0 = min((int)fx0, b.cw - 1);
  const int i1 = min((int)fy0 + 1, b.ch - 1), j1 = min((int)fx0 + 1, b.cw - 1);
  const float ly = in_y - fy0, lx = in_x - fx0;
  const int32_t* f = SHARED ? field : field + (int64_t)n * d.src_h * d.src_w;
  const int pitch = SHARED ? d.src_w : b.cw, oy = SHARED ? b.y1 : 0, ox = SHARED ? b.x1 : 0;
  const int dz = SHARED ? b.z1 + z - z0s[0] : z - z0s[n];
  const float tl = sp_at(f, pitch, oy + i0, ox + j0, dz, binary), tr = sp_at(f, pitch, oy + i0, ox + j1, dz, binary);
  const float bl = sp_at(f, pitch, oy + i1, ox + j0, dz, binary), br = sp_at(f, pitch, oy + i1, ox + j1, dz, binary);
  const float top = tl + (tr - tl) * lx, bot = bl + (br - bl) * lx;
  const float v = top + (bot - top) * ly;
  const int zo = t[9] != 0 ? d.D - 1 - z : z, yo = t[8] != 0 ? d.H - 1 - y : y, xo = t[7] != 0 ? d.W - 1 - x : x;
  const int64_t o = (int64_t)n * vol + ((int64_t)zo * d.H + yo) * d.W + xo;
  *reinterpret_cast<float2*>(img2 + o * 2) = make_float2(img1[o], v);
}

// ------------------------------------------------------------------------------------------------ host side
bool sp_valid(const unetk_lits3d_clicks_desc* d) {
  return d && d->N > 0 && d->N <= 65535 && d->D > 0 && d->H > 0 && d->W > 0 && d->n_slices > 0 && d->src_h > 0 && d->src_w > 0 &&
         d->lab_scale > 0 && d->obj_label > 0 && (int64_t)d->lab_scale * d->obj_label < ((int64_t)1 << 31);
}
bool sp_supported(const unetk_lits3d_clicks_desc* d) { return d->src_h <= SP_MAX_EXTENT && d->src_w <= SP_MAX_EXTENT; }
bool sp_mode_ok(int mode) { return mode == UNETK_SLICE_PRIOR_BOUNDARY || mode == UNETK_SLICE_PRIOR_BINARY; }

}  // namespace

extern "C" size_t unetk_slice_prior_ws_bytes(const unetk_lits3d_clicks_desc* d) {
  if (!sp_valid(d) || !sp_supported(d)) return 0;
  return (size_t)d->N * d->src_h * d->src_w * sizeof(int32_t);
}

extern "C" int unetk_slice_prior_field(const unetk_lits3d_clicks_desc* d, const uint8_t* seg_slices, const int32_t* sample_tab,
                                       const int32_t* pts, const int32_t* cnt, int K, int whole, int mode, int32_t* field,
                                       int32_t* z0, void* ws, size_t ws_bytes, void* stream) {
  UNETK_REQUIRE(sp_valid(d) && seg_slices && sample_tab && pts && cnt && field && z0 && sp_mode_ok(mode));
  UNETK_REQUIRE(K >= 0 && K <= UNETK_INTER_MAX_CLICKS);
  UNETK_REQUIRE(((((uintptr_t)sample_tab) | ((uintptr_t)pts) | ((uintptr_t)cnt) | ((uintptr_t)field) | ((uintptr_t)z0)) & 3u) == 0);
  if (!sp_supported(d)) return UNETK_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int binary = mode == UNETK_SLICE_PRIOR_BINARY;
  if (!binary) {
    UNETK_REQUIRE(ws && unetk_aligned16(ws));
    if (ws_bytes < unetk_slice_prior_ws_bytes(d)) return UNETK_E_WORKSPACE;
  }
  int32_t* gsq = static_cast<int32_t*>(ws);
  UNETK_LAUNCH(sp_rows_kernel, dim3(d->src_h, d->N), dim3(256), 0, st, *d, seg_slices, sample_tab, pts, cnt, K, whole != 0 ? 1 : 0,
               binary, binary ? field : gsq, z0);
  if (!binary)
    UNETK_LAUNCH(sp_cols_kernel, dim3((d->src_w + 63) / 64, (d->src_h + IEDT_T - 1) / IEDT_T, d->N), dim3(256), 0, st, *d, sample_tab,
                 (const int32_t*)z0, whole != 0 ? 1 : 0, (const int32_t*)gsq, field);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_slice_prior_render(const unetk_lits3d_clicks_desc* d, const int32_t* sample_tab, const float* images,
                                        const int32_t* field, const int32_t* z0, int shared, int mode, float* images2,
                                        void* stream) {
  UNETK_REQUIRE(d && d->N > 0 && d->D > 0 && d->H > 0 && d->W > 0 && d->src_h > 0 && d->src_w > 0 && sample_tab && images &&
                field && z0 && images2 && sp_mode_ok(mode));
  UNETK_REQUIRE(((((uintptr_t)sample_tab) | ((uintptr_t)images) | ((uintptr_t)field) | ((uintptr_t)z0)) & 3u) == 0);
  UNETK_REQUIRE((((uintptr_t)images2) & 7u) == 0);
  const int64_t total = (int64_t)d->N * d->D * d->H * d->W;
  if ((int64_t)d->D * d->H * d->W >= ((int64_t)1 << 31) || (total + 255) / 256 >= ((int64_t)1 << 31)) return UNETK_E_UNSUPPORTED;
  const dim3 grid((unsigned)((total + 255) / 256));
  const int binary = mode == UNETK_SLICE_PRIOR_BINARY;
  if (shared)
    UNETK_LAUNCH(sp_render_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *d, sample_tab, images, field, z0, binary, images2);
  else
    UNETK_LAUNCH(sp_render_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *d, sample_tab, images, field, z0, binary, images2);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}
