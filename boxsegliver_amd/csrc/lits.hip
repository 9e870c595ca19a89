// Training-batch assembly of the LiTS input pipeline on the device.
//
// The reference decodes three 16-bit PNG slices per sample on CPU threads and runs, per sample, inside tf.data:
// crop_to_bounding_box -> resize_bilinear(align_corners=True) -> clip to the window -> (x - lo) / (hi - lo), the label
// through crop -> resize_nearest_neighbor(align_corners=True) -> / LB_SCALE, then uniform noise (zero on padded
// slices) and random flips (DataLoader/Liver/input_pipeline.py:243-284; utils/image_ops.py).  On MI355X the decoded
// dataset (131 cases ~ 35 GB as uint16) simply LIVES in HBM; a step's batch is one kernel over the output pixels that
// gathers from the resident slices -- no host work, no host->device copy per step.
//   sample table row (int32): [slice index x C (-1 = zero padding slice), label slice index (-1 = zeros),
//                              off_y, off_x, crop_h, crop_w, flip_left_right, flip_up_down]
//   clip row (float):         [window lo, window hi]          (IM_SCALE units, input_pipeline.py:370-373)
// HBM-bound and tiny: reads <= 4 source pixels per output value.
#include "common.h"
#include "lits_geom.h"

namespace {

__device__ __forceinline__ float u01(uint32_t seed, uint64_t i) {   // counter-based: splitmix64 finaliser
  uint64_t z = (i + 0x9E3779B97F4A7C15ull) * 0xBF58476D1CE4E5B9ull + ((uint64_t)seed << 32 | seed);
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (float)(uint32_t)(z >> 40) * (1.0f / 16777216.0f);
}

__global__ __launch_bounds__(256) void lits_batch_kernel(unetk_lits_desc d, const uint16_t* __restrict__ slices,
                                                         const uint8_t* __restrict__ segs, const int32_t* __restrict__ tab,
                                                         const float* __restrict__ clip, float* __restrict__ images,
                                                         int32_t* __restrict__ labels) {
  const int64_t total = (int64_t)d.N * d.H * d.W;
  const int TW = d.C + 7;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % d.W);
    const int y = (int)((i / d.W) % d.H);
    const int n = (int)(i / ((int64_t)d.W * d.H));
    const int32_t* t = tab + (int64_t)n * TW;
    // a crop box outside the slice is a caller error (tf.image.crop_to_bounding_box raises); it is clamped into the
    // slice here so that it can never become an out-of-bounds read
    const int off_y = min(max(t[d.C + 1], 0), d.src_h - 1), off_x = min(max(t[d.C + 2], 0), d.src_w - 1);
    const int ch = min(max(t[d.C + 3], 1), d.src_h - off_y), cw = min(max(t[d.C + 4], 1), d.src_w - off_x);
    // random flips act on the finished sample: output (y, x) shows source position (sy, sx)
    const int sx = t[d.C + 5] ? d.W - 1 - x : x;
    const int sy = t[d.C + 6] ? d.H - 1 - y : y;
    // align_corners source coordinate and taps: lits_geom.h (shared with the 3-D patch kernel)
    const float in_y = sy * lits_ac_scale(ch, d.H), in_x = sx * lits_ac_scale(cw, d.W);
    const LitsTaps ty = lits_ac_taps(in_y, ch), tx = lits_ac_taps(in_x, cw);
    const int y0 = ty.i0, y1 = ty.i1, x0 = tx.i0, x1 = tx.i1;
    const float ly = ty.f, lx = tx.f;
    const float lo = clip[2 * n], hi = clip[2 * n + 1];
    const int64_t plane = (int64_t)d.src_h * d.src_w;
    for (int c = 0; c < d.C; ++c) {
      float v = 0.f;
      const int s = t[c];
      if (s >= 0 && s < d.n_slices) {
        const uint16_t* p = slices + s * plane + (int64_t)off_y * d.src_w + off_x;
        const float tl = p[(int64_t)y0 * d.src_w + x0], tr = p[(int64_t)y0 * d.src_w + x1];
        const float bl = p[(int64_t)y1 * d.src_w + x0], br = p[(int64_t)y1 * d.src_w + x1];
        v = lits_bilerp(tl, tr, bl, br, lx, ly);                              // tf resize_bilinear's lerp order
        v = (fminf(fmaxf(v, lo), hi) - lo) / (hi - lo);
        if (d.noise_scale > 0.f)   // noise is drawn per FINAL pixel (after the flip in the reference too)
          v += (2.f * u01(d.seed, ((uint64_t)i * d.C + c)) - 1.f) * d.noise_scale;
      }
      images[i * d.C + c] = v;
    }
    int lab = 0;
    const int ls = t[d.C];
    if (ls >= 0 && ls < d.n_slices) {
      const int ny = lits_ac_nearest(in_y, ch), nx = lits_ac_nearest(in_x, cw);
      lab = segs[ls * plane + (int64_t)(off_y + ny) * d.src_w + off_x + nx] / d.lab_scale;
    }
    labels[i] = lab;
  }
}

// Spatial guide of the guided pipeline (input_pipeline_g.py:382-412): the reference renders
// create_spatial_guide_2d(crop size, centres, max(stddevs, min_std)) per sample, resize_bilinear(align_corners) to the
// network size, then g / 2 + 0.5.  A bilinear resize of a rendered guide reads it at 4 integer corners, so each output pixel
// evaluates the Gaussians at exactly those corners -- the same arithmetic without the crop-resolution intermediate.  Sample
// geometry (crop clamp, flips, corners, weights) is lits_batch_kernel's, so guide and image line up pixel for pixel.
//   obj_ptr int32 [N + 1] (CSR into obj), obj float4 [n_obj] = (cy, cx, sy, sx), centres relative to the crop.
__device__ __forceinline__ float guide_at(float py, float px, const float4* __restrict__ o, int k0, int k1, float min_std) {
  float g = 0.f;                               // every term is >= 0: a max from 0 is create_spatial_guide_2d's reduce_max
  for (int k = k0; k < k1; ++k) {
    const float4 b = o[k];
    const float sy = fmaxf(b.z, min_std), sx = fmaxf(b.w, min_std);
    const float dy = py - b.x, dx = px - b.y;
    // (coords - center)^2 / (2 * s * s), summed y then x, full-precision exp (image_ops.py:396-434)
    g = fmaxf(g, expf(-(dy * dy / (2.f * sy * sy) + dx * dx / (2.f * sx * sx))));
  }
  return g;
}

__global__ __launch_bounds__(256) void lits_guide_kernel(unetk_lits_guide_desc d, const int32_t* __restrict__ tab,
                                                         const int32_t* __restrict__ obj_ptr, const float4* __restrict__ obj,
                                                         float* __restrict__ guide) {
  const int64_t total = (int64_t)d.N * d.H * d.W;
  const int TW = d.C + 7;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % d.W);
    const int y = (int)((i / d.W) % d.H);
    const int n = (int)(i / ((int64_t)d.W * d.H));
    // the CSR row is clamped into [0, n_obj]: a malformed pointer table cannot become an out-of-bounds read
    const int k0 = min(max(obj_ptr[n], 0), d.n_obj), k1 = min(max(obj_ptr[n + 1], k0), d.n_obj);
    if (k1 == k0) {              // no object on this sample: the reference's false_fn, exactly 0.5
      guide[i] = 0.5f;
      continue;
    }
    const int32_t* t = tab + (int64_t)n * TW;
    const int off_y = min(max(t[d.C + 1], 0), d.src_h - 1), off_x = min(max(t[d.C + 2], 0), d.src_w - 1);
    const int ch = min(max(t[d.C + 3], 1), d.src_h - off_y), cw = min(max(t[d.C + 4], 1), d.src_w - off_x);
    const int sx = t[d.C + 5] ? d.W - 1 - x : x;
    const int sy = t[d.C + 6] ? d.H - 1 - y : y;
    const float in_y = sy * lits_ac_scale(ch, d.H), in_x = sx * lits_ac_scale(cw, d.W);
    const LitsTaps ty = lits_ac_taps(in_y, ch), tx = lits_ac_taps(in_x, cw);
    const int y0 = ty.i0, y1 = ty.i1, x0 = tx.i0, x1 = tx.i1;
    const float ly = ty.f, lx = tx.f;
    const float tl = guide_at((float)y0, (float)x0, obj, k0, k1, d.min_std);
    const float tr = guide_at((float)y0, (float)x1, obj, k0, k1, d.min_std);
    const float bl = guide_at((float)y1, (float)x0, obj, k0, k1, d.min_std);
    const float br = guide_at((float)y1, (float)x1, obj, k0, k1, d.min_std);
    guide[i] = lits_bilerp(tl, tr, bl, br, lx, ly) / 2.f + 0.5f;         // tf resize_bilinear's lerp order
  }
}

// Guide of one slice of the propagation loop (input_pipeline_g.py:1427-1440): create_gaussian_distribution_v2 over the
// network-size image, times the discount, then / 2 + 0.5 -- guide_at's exp without the resize, stddevs taken as given (the
// host floors them at min_std).  No object: exactly 0.5.
__global__ __launch_bounds__(256) void guide_render_kernel(const float4* __restrict__ obj, int n_obj, int H, int W,
                                                           float discount, float* __restrict__ guide) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * W) return;
  if (n_obj == 0) {
    guide[i] = 0.5f;
    return;
  }
  const int y = i / W, x = i - (i / W) * W;
  const float g = guide_at((float)y, (float)x, obj, 0, n_obj, 0.f) * discount;
  guide[i] = g / 2.f + 0.5f;
}

// Context rows of a batch (input_pipeline_g.py:527-550, :672-680): sample s reads the resident row of its label slice
// (column C of the batch table); a failed coin or a padding slice (-1) gives zeros.  With noise (--hist_noise) the row is
// updated IN PLACE first, row = f32(f64(row) + noise[s]) -- the reference adds the noise into a view of its cached table --
// so the noise builds up over the run.  One thread per column walks the samples in order: a slice drawn twice in one
// batch takes both updates, the second sample sees the first one's result.
__global__ __launch_bounds__(256) void lits_context_kernel(float* __restrict__ table, int64_t n_rows, int F,
                                                           const int32_t* __restrict__ tab, int N, int C,
                                                           const int32_t* __restrict__ take, const double* __restrict__ noise,
                                                           float* __restrict__ out) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  for (int s = 0; s < N; ++s) {
    const int32_t idx = tab[(int64_t)s * (C + 7) + C];
    float v = 0.f;
    if (take[s] && idx >= 0 && idx < n_rows) {
      float* p = table + (int64_t)idx * F + f;
      v = *p;
      if (noise) {
        v = (float)((double)v + noise[(int64_t)s * F + f]);
        *p = v;
      }
    }
    out[(int64_t)s * F + f] = v;
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// PNG scanline un-filtering on the device (the loader of the resident slice store, data/lits.py).
//
// The reference decodes its PNG slices with cv2 on tf.data threads (DataLoader/Liver/input_pipeline.py:243-284; they were
// written by SimpleITK / libpng with ADAPTIVE row filters, DataLoader/Liver/extract.py:176-187).  Here the host only inflates
// the zlib stream (zlib releases the GIL: a thread pool scales) and uploads the FILTERED scanlines; this kernel undoes the
// five PNG filter types and writes native-endian pixels straight into the resident store.
//
// Every filter is  cur[i] = line[i] + pred(a, b, c)  mod 256 per byte lane, a = left pixel, b = the pixel above, c = above-left
// (None: 0, Sub: a, Up: b, Average: (a + b) >> 1, Paeth).  Average and Paeth chain through BOTH a (this row) and b (the row
// above), so the dependency is a wavefront: one wave per image, lane r owns row y0 + r of a 64-row band and runs ONE pixel
// behind lane r - 1 -- at step t it takes pixel i = t - r, its `b` is the value lane r - 1 produced at step t - 1 (a DPP
// shuffle), `c` its previous `b`, `a` its own previous output.  A band is w + 63 steps whatever mix of filter types its rows
// use; the band's last row goes through LDS to lane 0 of the next band (written at step i + 63, read at step i of the NEXT
// band).  Bytes in, bytes out: the host's inflate rate (a few thousand slices/s) is the pipeline's limit, not this kernel.
constexpr int PNG_MAX_W = 4096;

template <int BPP>
__global__ __launch_bounds__(64) void png_unfilter_kernel(const uint8_t* __restrict__ filt, int64_t in_stride, int h, int w,
                                                          void* __restrict__ out, int64_t out_stride, int32_t* __restrict__ status) {
  __shared__ uint8_t lastrow[PNG_MAX_W * BPP];
  const int lane = threadIdx.x;
  const uint8_t* src = filt + (int64_t)blockIdx.x * in_stride;
  const int rowb = w * BPP + 1;
  for (int i = lane; i < w * BPP; i += 64) lastrow[i] = 0;           // the row above row 0 is zero
  __syncthreads();
  for (int y0 = 0; y0 < h; y0 += 64) {
    const int y = y0 + lane;
    const bool active = y < h;
    const uint8_t* line = src + (int64_t)(active ? y : 0) * rowb;
    const int ft = active ? line[0] : 0;
    if (active && ft > 4) atomicOr(status, 1);                         // not a PNG filter type: the caller raises
    line += 1;
    const bool last_of_band = lane == 63 || y == h - 1;
    int a0 = 0, a1 = 0, c0 = 0, c1 = 0, o0 = 0, o1 = 0;
    for (int t = 0; t < w + 63; ++t) {
      const int i = t - lane;
      int b0 = __shfl_up(o0, 1), b1 = BPP == 2 ? __shfl_up(o1, 1) : 0;
      const bool on = active && i >= 0 && i < w;
      if (lane == 0 && on) {
        b0 = lastrow[i * BPP];
        if (BPP == 2) b1 = lastrow[i * BPP + 1];
      }
      if (on) {
        const int x0 = line[i * BPP], x1 = BPP == 2 ? line[i * BPP + 1] : 0;
        int p0 = 0, p1 = 0;
        if (ft == 1) { p0 = a0; p1 = a1; }
        else if (ft == 2) { p0 = b0; p1 = b1; }
        else if (ft == 3) { p0 = (a0 + b0) >> 1; p1 = (a1 + b1) >> 1; }
        else if (ft == 4) {
          const int q0 = a0 + b0 - c0, pa0 = abs(q0 - a0), pb0 = abs(q0 - b0), pc0 = abs(q0 - c0);
          p0 = (pa0 <= pb0 && pa0 <= pc0) ? a0 : (pb0 <= pc0 ? b0 : c0);
          const int q1 = a1 + b1 - c1, pa1 = abs(q1 - a1), pb1 = abs(q1 - b1), pc1 = abs(q1 - c1);
          p1 = (pa1 <= pb1 && pa1 <= pc1) ? a1 : (pb1 <= pc1 ? b1 : c1);
        }
        o0 = (x0 + p0) & 255;
        o1 = (x1 + p1) & 255;
        c0 = b0; c1 = b1; a0 = o0; a1 = o1;
        if (BPP == 2)      // PNG samples are big-endian
          static_cast<uint16_t*>(out)[(int64_t)blockIdx.x * out_stride + (int64_t)y * w + i] = (uint16_t)((o0 << 8) | o1);
        else
          static_cast<uint8_t*>(out)[(int64_t)blockIdx.x * out_stride + (int64_t)y * w + i] = (uint8_t)o0;
        if (last_of_band) {
          lastrow[i * BPP] = (uint8_t)o0;
          if (BPP == 2) lastrow[i * BPP + 1] = (uint8_t)o1;
        }
      }
    }
    __syncthreads();       // the band's last row is complete before the next band's lane 0 reads it
  }
}

extern "C" int unetk_png_unfilter(const uint8_t* filtered, int64_t image_stride_bytes, int n_images, int h, int w, int bit_depth,
                                  void* out, int64_t out_image_stride, int32_t* status, void* stream) {
  UNETK_REQUIRE(filtered && out && status && n_images > 0 && h > 0 && w > 0 && w <= PNG_MAX_W);
  UNETK_REQUIRE(bit_depth == 8 || bit_depth == 16);
  const int bpp = bit_depth / 8;
  UNETK_REQUIRE(image_stride_bytes >= (int64_t)h * (w * bpp + 1) && out_image_stride >= (int64_t)h * w);
  if (bpp == 2) {
    UNETK_REQUIRE((((uintptr_t)out) & 1u) == 0);
    UNETK_LAUNCH(png_unfilter_kernel<2>, dim3(n_images), dim3(64), 0, (hipStream_t)stream, filtered, image_stride_bytes, h, w, out,
                 out_image_stride, status);
  } else {
    UNETK_LAUNCH(png_unfilter_kernel<1>, dim3(n_images), dim3(64), 0, (hipStream_t)stream, filtered, image_stride_bytes, h, w, out,
                 out_image_stride, status);
  }
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_lits_batch(const unetk_lits_desc* d, const uint16_t* slices, const uint8_t* seg_slices,
                                const int32_t* sample_tab, const float* clip, float* images, int32_t* labels,
                                void* stream) {
  UNETK_REQUIRE(d && slices && seg_slices && sample_tab && clip && images && labels);
  UNETK_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->C <= 8 && d->src_h > 0 && d->src_w > 0 && d->lab_scale > 0);
  const int64_t total = (int64_t)d->N * d->H * d->W;
  int64_t grid = (total + 255) / 256;
  if (grid > 65536) grid = 65536;
  UNETK_LAUNCH(lits_batch_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, *d, slices, seg_slices,
                     sample_tab, clip, images, labels);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_lits_spatial_guide(const unetk_lits_guide_desc* d, const int32_t* sample_tab, const int32_t* obj_ptr,
                                        const float* obj, float* guide, void* stream) {
  UNETK_REQUIRE(d && sample_tab && obj_ptr && guide && (obj || d->n_obj == 0));
  UNETK_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->C <= 8 && d->src_h > 0 && d->src_w > 0 && d->n_obj >= 0);
  UNETK_REQUIRE(d->min_std > 0.f);                    // a zero stddev would divide by zero (image_ops.py: "must not contain zero")
  UNETK_REQUIRE(d->n_obj == 0 || (((uintptr_t)obj) & 15u) == 0);       // float4 rows
  const int64_t total = (int64_t)d->N * d->H * d->W;
  int64_t grid = (total + 255) / 256;
  if (grid > 65536) grid = 65536;
  UNETK_LAUNCH(lits_guide_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, *d, sample_tab, obj_ptr,
               reinterpret_cast<const float4*>(obj), guide);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_lits_context(float* table, int64_t n_rows, int F, const int32_t* sample_tab, int N, int C,
                                  const int32_t* take, const double* noise, float* out, void* stream) {
  UNETK_REQUIRE(table && sample_tab && take && out && n_rows > 0 && F > 0 && N > 0 && C > 0 && C <= 8);
  UNETK_REQUIRE(noise == nullptr || (((uintptr_t)noise) & 7u) == 0);
  UNETK_LAUNCH(lits_context_kernel, dim3((F + 255) / 256), dim3(256), 0, (hipStream_t)stream, table, n_rows, F, sample_tab, N, C,
               take, noise, out);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_guide_render(const float* obj, int n_obj, int H, int W, float discount, float* guide, void* stream) {
  UNETK_REQUIRE(guide && H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31) && n_obj >= 0 && (obj || n_obj == 0));
  UNETK_REQUIRE(n_obj == 0 || (((uintptr_t)obj) & 15u) == 0);
  const int64_t total = (int64_t)H * W;
  UNETK_LAUNCH(guide_render_kernel, dim3((int)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
               reinterpret_cast<const float4*>(obj), n_obj, H, W, discount, guide);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}
