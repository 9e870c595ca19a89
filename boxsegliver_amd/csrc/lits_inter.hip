// Click-guided 2-D batches for UNetInter / SmallUNet / InterUNet / LGNet from the resident LiTS slice store.
//
// The semantics are those of the reference's interactive pipeline for the NF data (DataLoader/NF/input_pipeline_g_simply.py:
// :564-636 gen_batch, :435-527 data_processing, :346-412 inter_simulation as :530-561 gen_kernel calls it; DataLoader/misc.py:
// 108-129 img_crop; utils/image_ops.py:396-434 create_spatial_guide_2d), the volumes are the cases of data/lits.SliceStore and the
// sample table is the LiTS 3-D one (include/unetk.h), so unetk_lits_pick_voxel centres the forced samples on the device.
//   unetk_lits_inter_batch  crop [C, ch, cw] -> z-score over its non-zero voxels -> resize_bilinear(align_corners) -> flips ->
//                           (training) gamma with retain_stats, uniform noise, channel mask; labels nearest, {0, 1}
//   unetk_lits_clicks       inter_simulation on the label crop at source resolution: the reference runs it in a pool of host
//                           processes; the labels live here, so it runs here
//   unetk_click_guide       create_spatial_guide_2d + resize_bilinear from the clicks, evaluated at the bilinear corners
//   unetk_click_guide_list  the same kernel on lists of K <= 64 clicks per kind (the interactive evaluator)
//
// The click simulator.  binary_erosion(mask, iterations=m) with the default cross is "city-block distance to the nearest 0
// > m", so both candidate sets come from ONE capped distance transform per kind instead of 3 + 40 erosion sweeps:
//   clk_cols_kernel   thread per crop column: distance along the column to the nearest non-object pixel (foreground; the
//                     crop's border counts) and to the nearest object pixel (background), two sweeps, capped at
//                     margin + band + 1 <= 255 -> two byte fields
//   clk_rows_kernel   block per crop row, the row in LDS: d(x) = min_x' g(x') + |x - x'| by min-plus doubling (offsets 1, 2, 4,
//                     ... compose every |x - x'| below the cap exactly) -> one byte per pixel: candidate of the foreground,
//                     candidate of the background, object
//   clk_select_kernel block per (sample, kind): counts, ranks and arg-maxima over the class bytes; the suppression after a
//                     click is not written back, a candidate is alive while it is farther than `step` from every click so far
// Everything is integer arithmetic and every reduction has a fixed order (ballots inside a wave, waves by index).
#include "common.h"
#include "lits_clicks.h"     // MAXK, CTW, CLS_*, CLK_U, clk_draws, clk_col_sweeps, clk_row_minplus: shared with the other simulators
#include "lits_geom.h"
#include "lits_inter_px.h"  // Box2, ib_box, ib_slice, ib_mask_stats_kernel, ib_value, ib_valid: shared with lits_geodesic.hip
#include "lits_patch.h"

namespace {

// ------------------------------------------------------------------------------------------------ images: the patch
// Pixel (y, x) of the resized, un-flipped sample, all channels; the flips are its write address.
__global__ __launch_bounds__(256) void ib_patch_kernel(unetk_lits_inter_desc d, const uint16_t* __restrict__ slices,
                                                       const uint8_t* __restrict__ segs, const int32_t* __restrict__ tab,
                                                       const float* __restrict__ stat, float* __restrict__ images,
                                                       int32_t* __restrict__ labels, int32_t* __restrict__ status,
                                                       double* __restrict__ part, float* __restrict__ minmax) {
  const int n = blockIdx.y, P = gridDim.x;
  const int32_t* t = tab + (int64_t)n * TW;
  const Box2 b = ib_box(t, d);
  const bool flr = t[7] != 0, fud = t[8] != 0;
  const float m = stat[(int64_t)n * ST_N + ST_M], den = stat[(int64_t)n * ST_N + ST_S] + 1e-8f;
  const float scale = (float)d.im_scale;
  const float hs = lits_ac_scale(b.ch, d.H), ws = lits_ac_scale(b.cw, d.W);
  const int64_t plane = (int64_t)d.src_h * d.src_w;
  const int area = d.H * d.W;
  const int thr = d.obj_label * d.lab_scale;                 // seg / lab_scale >= obj  <=>  seg >= obj * lab_scale
  const int64_t sl = ib_slice(b, 0, d);
  if (sl < 0 && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 2);
  float* img = images + (int64_t)n * area * d.C;
  int32_t* lab = labels + (int64_t)n * area;
  double cnt = 0., sum = 0., sq = 0.;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < area; i += P * 256) {
    const int y = i / d.W, x = i - y * d.W;
    const float in_y = y * hs, in_x = x * ws;
    const IbTaps tp = ib_taps(y, x, b, hs, ws);
    const int yo = fud ? d.H - 1 - y : y, xo = flr ? d.W - 1 - x : x;
    const int o = yo * d.W + xo;
    for (int c = 0; c < d.C; ++c) {
      float v = 0.f;
      const int64_t s = ib_slice(b, c - d.C / 2, d);
      if (s >= 0) v = ib_value(slices + s * plane + (int64_t)b.y1 * d.src_w + b.x1, d.src_w, tp, scale, m, den);
      img[(int64_t)o * d.C + c] = v;
      cnt += 1.;
      sum += (double)v;
      sq += (double)v * (double)v;
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
    int l = 0;
    if (sl >= 0) {
      const int ny = lits_ac_nearest(in_y, b.ch), nx = lits_ac_nearest(in_x, b.cw);
      l = (int)segs[sl * plane + (int64_t)(b.y1 + ny) * d.src_w + b.x1 + nx] >= thr ? 1 : 0;
    }
    lab[o] = l;
  }
  if (d.training) {
    block_sum3(cnt, sum, sq, part + ((int64_t)n * P + blockIdx.x) * 3);
    block_minmax(lo, hi, minmax + ((int64_t)n * P + blockIdx.x) * 2);
  }
}

// ------------------------------------------------------------------------------------------------ images: noise, channel mask
// image_ops.py:209-238 random_noise with the library's counter generator: every operation rounded on its own, so that the
// result is the float32 sum a restatement forms
__device__ __forceinline__ float ib_noised(float v, float u, float s) {
#pragma clang fp contract(off)
  const float t = 2.f * u - 1.f;
  const float nz = t * s;
  return v + nz;
}
__global__ __launch_bounds__(256) void ib_noise_kernel(unetk_lits_inter_desc d, float* __restrict__ images,
                                                       float* __restrict__ cmax) {
  __shared__ float sh[4][8];
  const int n = blockIdx.y, P = gridDim.x;
  const int area = d.H * d.W;
  float* img = images + (int64_t)n * area * d.C;
  float mx[IB_MAX_C];
#pragma unroll
  for (int c = 0; c < IB_MAX_C; ++c) mx[c] = -INFINITY;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < area; i += P * 256) {
#pragma unroll
    for (int c = 0; c < IB_MAX_C; ++c) {
      if (c < d.C) {
        const int64_t e = ((int64_t)n * area + i) * d.C + c;
        const float v = ib_noised(img[(int64_t)i * d.C + c], unetk_uniform(d.seed, (uint32_t)e), d.noise_scale);
        img[(int64_t)i * d.C + c] = v;
        mx[c] = fmaxf(mx[c], v);
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < IB_MAX_C; ++c) {
    float v = mx[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if (lane == 0) sh[wave][c] = v;
  }
  __syncthreads();
  if (threadIdx.x < IB_MAX_C)
    cmax[((int64_t)n * P + blockIdx.x) * 8 + threadIdx.x] =
        fmaxf(fmaxf(sh[0][threadIdx.x], sh[1][threadIdx.x]), fmaxf(sh[2][threadIdx.x], sh[3][threadIdx.x]));
}
// data_processing :524: images *= float(reduce_max(images, axis=(0, 1)) > 0)
__global__ __launch_bounds__(256) void ib_chmask_kernel(unetk_lits_inter_desc d, const float* __restrict__ cmax,
                                                        float* __restrict__ images) {
  __shared__ float keep[8];
  const int n = blockIdx.y, P = gridDim.x;
  if (threadIdx.x < IB_MAX_C) {
    float v = -INFINITY;
    for (int p = 0; p < P; ++p) v = fmaxf(v, cmax[((int64_t)n * P + p) * 8 + threadIdx.x]);
    keep[threadIdx.x] = v > 0.f ? 1.f : 0.f;
  }
  __syncthreads();
  const int total = d.H * d.W * d.C;
  float* img = images + (int64_t)n * total;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += P * 256) img[i] *= keep[i % d.C];
}

// ------------------------------------------------------------------------------------------------ clicks: column distances
// gf = distance along the column to the nearest non-object pixel, the crop's border counting as one (0 on non-object
// pixels); gb = distance along the column to the nearest object pixel; both capped at `cap`.  Indexed y * cw + x.
__global__ __launch_bounds__(64) void clk_cols_kernel(unetk_lits_inter_desc d, const uint8_t* __restrict__ segs,
                                                      const int32_t* __restrict__ tab, uint8_t* __restrict__ ws,
                                                      int32_t* __restrict__ status) {
  const int n = blockIdx.y, x = blockIdx.x * 64 + threadIdx.x;
  const Box2 b = ib_box(tab + (int64_t)n * TW, d);
  const int64_t plane = (int64_t)d.src_h * d.src_w;
  const int64_t sl = ib_slice(b, 0, d);
  if (sl < 0 && x == 0) atomicOr(status, 2);
  if (x >= b.cw) return;
  const int cap = d.margin + d.band + 1, thr = d.obj_label * d.lab_scale;
  uint8_t* gf = ws + (int64_t)n * 3 * plane;
  uint8_t* gb = gf + plane;
  const uint8_t* p = segs + (sl < 0 ? 0 : sl) * plane + (int64_t)b.y1 * d.src_w + b.x1 + x;
  clk_col_sweeps(p, sl >= 0, d.src_w, b.ch, b.cw, thr, cap, gf + x, gb + x);
}

// ------------------------------------------------------------------------------------------------ clicks: row pass, classes
__global__ __launch_bounds__(256) void clk_rows_kernel(unetk_lits_inter_desc d, const int32_t* __restrict__ tab,
                                                       uint8_t* __restrict__ ws) {
  __shared__ int16_t buf[2][2][CLK_MAX_EXTENT];
  const int n = blockIdx.y, y = blockIdx.x;
  const Box2 b = ib_box(tab + (int64_t)n * TW, d);
  if (y >= b.ch) return;                                     // block-uniform
  const int64_t plane = (int64_t)d.src_h * d.src_w;
  const int cap = d.margin + d.band + 1, cw = b.cw;
  const uint8_t* gf = ws + (int64_t)n * 3 * plane + (int64_t)y * cw;
  const uint8_t* gb = gf + plane;
  uint8_t* cls = ws + (int64_t)n * 3 * plane + 2 * plane + (int64_t)y * cw;
  for (int x = threadIdx.x; x < cw; x += 256) {
    buf[0][0][x] = (int16_t)min((int)gf[x], min(x + 1, cw - x));          // the crop's left and right border: border_value = 0
    buf[0][1][x] = (int16_t)gb[x];
  }
  __syncthreads();
  const int cur = clk_row_minplus<2>(buf, cw, cap);
  for (int x = threadIdx.x; x < cw; x += 256) {
    const int df = buf[cur][0][x], db = buf[cur][1][x];
    cls[x] = (uint8_t)((df > d.margin ? CLS_FG : 0) | ((db > d.margin && db <= d.margin + d.band) ? CLS_BG : 0) |
                       (df > 0 ? CLS_OBJ : 0));
  }
}

// ------------------------------------------------------------------------------------------------ clicks: selection
struct Clicks {
  int n, y[MAXK], x[MAXK];
};
// a candidate is alive while it lies farther than `step` from every click so far (inter_simulation :401-408)
__device__ __forceinline__ bool clk_alive(int cls, int bit, int y, int x, const Clicks& c, int step2) {
  bool a = (cls & bit) != 0;
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {                           // unrolled: the clicks stay in registers
    const int dy = y - c.y[k], dx = x - c.x[k];
    a = a && (k >= c.n || dy * dy + dx * dx > step2);
  }
  return a;
}
__global__ __launch_bounds__(1024) void clk_select_kernel(unetk_lits_inter_desc d, const int32_t* __restrict__ tab,
                                                          const uint32_t* __restrict__ click_tab,
                                                          const uint8_t* __restrict__ ws, int32_t* __restrict__ pts,
                                                          int32_t* __restrict__ cnt, int32_t* __restrict__ status) {
  __shared__ unsigned long long red[16][3];
  __shared__ unsigned long long wbest[16];
  __shared__ int wcnt[16];
  __shared__ int pick[2];
  const int kind = blockIdx.x, n = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Box2 b = ib_box(tab + (int64_t)n * TW, d);
  const int64_t plane = (int64_t)d.src_h * d.src_w;
  const uint8_t* cls = ws + (int64_t)n * 3 * plane + 2 * plane;
  const int cw = b.cw, total = b.ch * b.cw;
  const int chunk = ((total + 15) / 16 + 63) / 64 * 64;      // pixels of a wave: a multiple of 64, row-major order across waves
  const int lo = min(wave * chunk, total), hi = min(lo + chunk, total);
  const int bit = kind == 0 ? CLS_FG : CLS_BG, step2 = d.step * d.step;
  // the sample's draws, clamped into their ranges
  const uint32_t* ct = click_tab + (int64_t)n * CTW;
  const ClkDraws dr = clk_draws(ct, kind, d.max_clicks);
  const int want = dr.want, strategy = dr.strategy;
  if (threadIdx.x == 0 && dr.bad) atomicOr(status, 4);

  // pass 0: candidates per wave; the mask's pixel count and coordinate sums
  Clicks c;
  c.n = 0;
#pragma unroll
  for (int k = 0; k < MAXK; ++k) c.y[k] = c.x[k] = 0;
  const float rcw = 1.f / (float)cw;                         // i / cw through unetk_fdiv: i < 2^20 + 512
  int ncand = 0;
  unsigned long long nmask = 0, sy = 0, sx = 0;
  for (int i0 = lo; i0 < hi; i0 += 64 * CLK_U) {            // wave-uniform trip count: the ballots see whole waves
    int v[CLK_U];
#pragma unroll
    for (int u = 0; u < CLK_U; ++u) v[u] = i0 + u * 64 + lane < hi ? (int)cls[i0 + u * 64 + lane] : 0;
#pragma unroll
    for (int u = 0; u < CLK_U; ++u) {
      const int i = i0 + u * 64 + lane;
      ncand += __popcll(__ballot((v[u] & bit) != 0));
      if (i < hi && ((v[u] & CLS_OBJ) != 0) == (kind == 0)) {
        const int y = unetk_fdiv(i, cw, rcw);
        nmask += 1;
        sy += (unsigned long long)y;
        sx += (unsigned long long)(i - y * cw);
      }
    }
  }
  nmask = wave_sum(nmask);
  sy = wave_sum(sy);
  sx = wave_sum(sx);
  if (lane == 0) {
    wcnt[wave] = ncand;
    red[wave][0] = nmask;
    red[wave][1] = sy;
    red[wave][2] = sx;
  }
  __syncthreads();
  nmask = sy = sx = 0;
  for (int w = 0; w < 16; ++w) {
    nmask += red[w][0];
    sy += red[w][1];
    sx += red[w][2];
  }
  int alive = 0;
  for (int w = 0; w < 16; ++w) alive += wcnt[w];

  if (nmask == 0 || want == 0) {
    // no pixel to click on (deviation: the reference fails on an all-object crop), or no click drawn
  } else if (alive == 0) {                                   // "small": one click at the mask's mean, floored
    c.y[0] = (int)(sy / nmask);
    c.x[0] = (int)(sx / nmask);
    c.n = 1;
  } else {
    for (int k = 0; k < want; ++k) {
      if (k > 0) {                                           // what the clicks so far leave
        __syncthreads();                                     // wcnt, pick and wbest are read above / below
        int a = 0;
        for (int i0 = lo; i0 < hi; i0 += 64 * CLK_U) {
          int v[CLK_U];
#pragma unroll
          for (int u = 0; u < CLK_U; ++u) v[u] = i0 + u * 64 + lane < hi ? (int)cls[i0 + u * 64 + lane] : 0;
#pragma unroll
          for (int u = 0; u < CLK_U; ++u) {
            const int i = i0 + u * 64 + lane, y = unetk_fdiv(i, cw, rcw);
            a += __popcll(__ballot(clk_alive(v[u], bit, y, i - y * cw, c, step2)));
          }
        }
        if (lane == 0) wcnt[wave] = a;
        __syncthreads();
        alive = 0;
        for (int w = 0; w < 16; ++w) alive += wcnt[w];
        if (alive == 0) break;                               // block-uniform
      }
      if (k == 0 || strategy == 1) {
        // rank i = (r * count) >> 32 in row-major order: the wave that holds it walks its pixels ballot by ballot
        int rank = (int)(((unsigned long long)ct[4 + 4 * kind + k] * (unsigned long long)alive) >> 32);
        int w0 = 0;
        while (rank >= wcnt[w0]) rank -= wcnt[w0++];         // rank < alive = sum of wcnt: ends inside the array
        if (wave == w0) {
          bool found = false;                                // wave-uniform
          for (int i0 = lo; i0 < hi && !found; i0 += 64 * CLK_U) {
            int v[CLK_U];
#pragma unroll
            for (int u = 0; u < CLK_U; ++u) v[u] = i0 + u * 64 + lane < hi ? (int)cls[i0 + u * 64 + lane] : 0;
#pragma unroll
            for (int u = 0; u < CLK_U; ++u) {
              if (found) continue;
              const int i = i0 + u * 64 + lane, y = unetk_fdiv(i, cw, rcw), x = i - y * cw;
              const bool a = clk_alive(v[u], bit, y, x, c, step2);
              const unsigned long long m = __ballot(a);
              const int here = __popcll(m);
              if (rank < here) {
                if (a && __popcll(m & ((1ull << lane) - 1ull)) == rank) {
                  pick[0] = y;
                  pick[1] = x;
                }
                found = true;
              } else {
                rank -= here;
              }
            }
          }
        }
      } else {
        // strategy 3: the candidate farthest from the clicks so far, the first in row-major order on ties (np.argmax)
        unsigned long long best = 0;
        for (int i0 = lo; i0 < hi; i0 += 64 * CLK_U) {
          int v[CLK_U];
#pragma unroll
          for (int u = 0; u < CLK_U; ++u) v[u] = i0 + u * 64 + lane < hi ? (int)cls[i0 + u * 64 + lane] : 0;
#pragma unroll
          for (int u = 0; u < CLK_U; ++u) {
            const int i = i0 + u * 64 + lane, y = unetk_fdiv(i, cw, rcw), x = i - y * cw;
            if (!clk_alive(v[u], bit, y, x, c, step2)) continue;
            unsigned int d2 = 0xffffffffu;
#pragma unroll
            for (int j = 0; j < MAXK; ++j) {
              const int dy = y - c.y[j], dx = x - c.x[j];
              d2 = j < c.n ? min(d2, (unsigned int)(dy * dy + dx * dx)) : d2;
            }
            const unsigned long long key = unetk_first_key(d2, (unsigned int)i);
            best = key > best ? key : best;
          }
        }
        best = wave_max(best);
        if (lane == 0) wbest[wave] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
          for (int w = 0; w < 16; ++w) best = wbest[w] > best ? wbest[w] : best;
          const int i = unetk_key_index(best);
          pick[0] = i / cw;
          pick[1] = i - (i / cw) * cw;
        }
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < MAXK; ++j) {
        if (j == c.n) {
          c.y[j] = pick[0];
          c.x[j] = pick[1];
        }
      }
      c.n += 1;
    }
  }
  if (threadIdx.x == 0) {
    int32_t* o = pts + ((int64_t)n * 2 + kind) * MAXK * 2;
#pragma unroll
    for (int k = 0; k < MAXK; ++k) {
      o[2 * k + 0] = k < c.n ? c.y[k] : -1;
      o[2 * k + 1] = k < c.n ? c.x[k] : -1;
    }
  }
  if (threadIdx.x == 0) cnt[(int64_t)n * 2 + kind] = c.n;
}

// ------------------------------------------------------------------------------------------------ guide
// create_spatial_guide_2d at one crop pixel: min_k sqrt(dy^2 + dx^2) = sqrt(min_k ...) (the squares are exact integers),
// or max_k exp(-(dy^2 / (2 s^2) + dx^2 / (2 s^2))) summed y then x as image_ops.py:433 sums them
__device__ __forceinline__ float cg_at(int py, int px, const int32_t* __restrict__ p, int n, bool gaussian, float two_s2) {
  if (n == 0) return 0.f;
  float best = gaussian ? 0.f : INFINITY;
  for (int k = 0; k < n; ++k) {
    const float dy = (float)py - (float)p[2 * k], dx = (float)px - (float)p[2 * k + 1];
    if (gaussian)
      best = fmaxf(best, expf(-(dy * dy / two_s2 + dx * dx / two_s2)));
    else
      best = fminf(best, dy * dy + dx * dx);
  }
  return gaussian ? best : sqrtf(best);
}
__global__ __launch_bounds__(256) void click_guide_kernel(unetk_lits_inter_desc d, const int32_t* __restrict__ tab,
                                                          const int32_t* __restrict__ pts, const int32_t* __restrict__ cnt,
                                                          int K, float* __restrict__ guide) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int area = d.H * d.W;
  if (i >= (int64_t)d.N * area) return;
  const int n = (int)(i / area), r = (int)(i - (int64_t)n * area);
  const int y = r / d.W, x = r - y * d.W;
  const int32_t* t = tab + (int64_t)n * TW;
  const Box2 b = ib_box(t, d);
  const LitsTaps ty = lits_ac_taps(y * lits_ac_scale(b.ch, d.H), b.ch), tx = lits_ac_taps(x * lits_ac_scale(b.cw, d.W), b.cw);
  const int y0 = min(ty.i0, b.ch - 1), x0 = min(tx.i0, b.cw - 1);
  const bool gaussian = d.gaussian != 0;
  const float two_s2 = 2.f * d.stddev * d.stddev;
  float g[2];
#pragma unroll
  for (int kind = 0; kind < 2; ++kind) {
    const int32_t* p = pts + ((int64_t)n * 2 + kind) * K * 2;  // K clicks per list: MAXK, or the evaluator's --max_iter
    const int k = min(max(cnt[(int64_t)n * 2 + kind], 0), K);
    const float tl = cg_at(y0, x0, p, k, gaussian, two_s2), tr = cg_at(y0, tx.i1, p, k, gaussian, two_s2);
    const float bl = cg_at(ty.i1, x0, p, k, gaussian, two_s2), br = cg_at(ty.i1, tx.i1, p, k, gaussian, two_s2);
    g[kind] = lits_bilerp(tl, tr, bl, br, tx.f, ty.f);
  }
  const int yo = t[8] != 0 ? d.H - 1 - y : y, xo = t[7] != 0 ? d.W - 1 - x : x;
  const int64_t o = (int64_t)n * area + (int64_t)yo * d.W + xo;
  if (d.G == 2) {
    guide[o * 2 + 0] = g[0];
    guide[o * 2 + 1] = g[1];
  } else {
    guide[o] = g[0] - g[1];
  }
}

// ------------------------------------------------------------------------------------------------ host side
bool clk_supported(const unetk_lits_inter_desc* d) {
  return d->margin >= 1 && d->band >= 1 && d->step >= 0 && d->step <= 16384 && (int64_t)d->margin + d->band <= 254 &&
         d->max_clicks >= 2 && d->max_clicks <= MAXK + 1 && d->src_h <= CLK_MAX_EXTENT && d->src_w <= CLK_MAX_EXTENT;
}

}  // namespace

extern "C" size_t unetk_lits_inter_batch_ws_bytes(const unetk_lits_inter_desc* d) {
  if (!ib_valid(d) || !ib_supported(d)) return 0;
  return (size_t)d->N * ib_blocks(d) * (3 * sizeof(double) + 2 * sizeof(float) + 8 * sizeof(float)) +
         (size_t)d->N * ST_N * sizeof(float);
}

extern "C" int unetk_lits_inter_batch(const unetk_lits_inter_desc* d, const uint16_t* slices, const uint8_t* seg_slices,
                                      const int32_t* sample_tab, float* images, int32_t* labels, int32_t* status, void* ws,
                                      size_t ws_bytes, void* stream) {
  UNETK_REQUIRE(ib_valid(d) && slices && seg_slices && sample_tab && images && labels && status && ws);
  UNETK_REQUIRE((((uintptr_t)slices) & 1u) == 0 &&
                ((((uintptr_t)sample_tab) | ((uintptr_t)images) | ((uintptr_t)labels) | ((uintptr_t)status)) & 3u) == 0);
  UNETK_REQUIRE(unetk_aligned16(ws) && d->noise_scale >= 0.f);
  if (!ib_supported(d)) return UNETK_E_UNSUPPORTED;
  if (ws_bytes < unetk_lits_inter_batch_ws_bytes(d)) return UNETK_E_WORKSPACE;
  const int P = ib_blocks(d);
  double* part = static_cast<double*>(ws);
  float* minmax = reinterpret_cast<float*>(part + (size_t)d->N * P * 3);
  float* stat = minmax + (size_t)d->N * P * 2;
  float* cmax = stat + (size_t)d->N * ST_N;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(P, d->N), fin(d->N);
  UNETK_LAUNCH(ib_mask_stats_kernel, grid, dim3(256), 0, st, *d, slices, sample_tab, part);
  UNETK_LAUNCH(p3d_finalize_kernel, fin, dim3(64), 0, st, 0, P, (const double*)part, (const float*)minmax, stat);
  UNETK_LAUNCH(ib_patch_kernel, grid, dim3(256), 0, st, *d, slices, seg_slices, sample_tab, (const float*)stat, images, labels,
               status, part, minmax);
  if (d->training) {
    const int total = d->H * d->W * d->C;                      // < 2^31: ib_supported
    UNETK_LAUNCH(p3d_finalize_kernel, fin, dim3(64), 0, st, 1, P, (const double*)part, (const float*)minmax, stat);
    UNETK_LAUNCH(p3d_gamma_kernel, grid, dim3(256), 0, st, total, sample_tab, (const float*)stat, images, part);
    UNETK_LAUNCH(p3d_finalize_kernel, fin, dim3(64), 0, st, 2, P, (const double*)part, (const float*)minmax, stat);
    UNETK_LAUNCH(p3d_retain_kernel, grid, dim3(256), 0, st, total, (const float*)stat, images);
    if (d->noise_scale > 0.f) {
      UNETK_LAUNCH(ib_noise_kernel, grid, dim3(256), 0, st, *d, images, cmax);
      UNETK_LAUNCH(ib_chmask_kernel, grid, dim3(256), 0, st, *d, (const float*)cmax, images);
    }
  }
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" size_t unetk_lits_clicks_ws_bytes(const unetk_lits_inter_desc* d) {
  if (!ib_valid(d) || !clk_supported(d)) return 0;
  return ((size_t)d->N * 3 * d->src_h * d->src_w + 15) / 16 * 16;
}

extern "C" int unetk_lits_clicks(const unetk_lits_inter_desc* d, const uint8_t* seg_slices, const int32_t* sample_tab,
                                 const uint32_t* click_tab, int32_t* pts, int32_t* cnt, int32_t* status, void* ws,
                                 size_t ws_bytes, void* stream) {
  UNETK_REQUIRE(ib_valid(d) && seg_slices && sample_tab && click_tab && pts && cnt && status && ws);
  UNETK_REQUIRE(((((uintptr_t)sample_tab) | ((uintptr_t)click_tab) | ((uintptr_t)pts) | ((uintptr_t)cnt) | ((uintptr_t)status)) & 3u) == 0);
  if (!clk_supported(d)) return UNETK_E_UNSUPPORTED;
  if (ws_bytes < unetk_lits_clicks_ws_bytes(d)) return UNETK_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  uint8_t* w = static_cast<uint8_t*>(ws);
  UNETK_LAUNCH(clk_cols_kernel, dim3((d->src_w + 63) / 64, d->N), dim3(64), 0, st, *d, seg_slices, sample_tab, w, status);
  UNETK_LAUNCH(clk_rows_kernel, dim3(d->src_h, d->N), dim3(256), 0, st, *d, sample_tab, w);
  UNETK_LAUNCH(clk_select_kernel, dim3(2, d->N), dim3(1024), 0, st, *d, sample_tab, click_tab, (const uint8_t*)w, pts, cnt, status);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

static int click_guide_run(const unetk_lits_inter_desc* d, const int32_t* sample_tab, const int32_t* pts, const int32_t* cnt,
                           int K, float* guide, void* stream) {
  UNETK_REQUIRE(ib_valid(d) && sample_tab && pts && cnt && guide && (d->G == 1 || d->G == 2));
  UNETK_REQUIRE(((((uintptr_t)sample_tab) | ((uintptr_t)pts) | ((uintptr_t)cnt) | ((uintptr_t)guide)) & 3u) == 0);
  UNETK_REQUIRE(d->gaussian == 0 || d->stddev > 0.f);
  const int64_t total = (int64_t)d->N * d->H * d->W;
  if ((int64_t)d->H * d->W >= ((int64_t)1 << 31) || (total + 255) / 256 >= ((int64_t)1 << 31)) return UNETK_E_UNSUPPORTED;
  UNETK_LAUNCH(click_guide_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *d, sample_tab, pts,
               cnt, K, guide);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_click_guide(const unetk_lits_inter_desc* d, const int32_t* sample_tab, const int32_t* pts,
                                 const int32_t* cnt, float* guide, void* stream) {
  return click_guide_run(d, sample_tab, pts, cnt, MAXK, guide, stream);
}

// the same guide from lists of K clicks per kind (the interactive evaluator's): one kernel, one arithmetic
extern "C" int unetk_click_guide_list(const unetk_lits_inter_desc* d, const int32_t* sample_tab, const int32_t* pts,
                                      const int32_t* cnt, int K, float* guide, void* stream) {
  UNETK_REQUIRE(K >= 1 && K <= UNETK_INTER_MAX_CLICKS);
  return click_guide_run(d, sample_tab, pts, cnt, K, guide, stream);
}
