// Input and output side of the offline volume evaluation (data/lits.py get_dataset_for_eval_image[_v2],
// evaluators/evaluator_liver.py _predict_case): the network's input slabs are built from a case's resident HU crop, and
// the argmax volume is zoomed back to the crop's shape, without the volume crossing to the host in between.  Both kernels
// are gathers: every output element is written exactly once, by plain stores, no atomics and no workspace.
//
// Threads walk the FLAT output (the contiguous axis fastest): a thread owns V consecutive elements = one 16-byte store,
// decomposes the index of its first element once (32-bit divisions) and steps the coordinates with carries, so 16-byte
// stores do not need rows of a suitable length; a base pointer that is not 16-byte aligned takes the one-element variant,
// and the elements past the last whole group are stored one by one.
#include "common.h"

// hipcc contracts a * b + c into an FMA by default, also through __fmul_rn / __fadd_rn (plain operators in its headers):
// the host rule rounds every product and sum on its own (numpy float32), so contraction is switched off for this file.
#pragma clang fp contract(off)

namespace {

constexpr int EIO_BLOCK = 256;
constexpr int EIO_ITERS = 4;                 // groups per thread: amortises the window table's trip into LDS
constexpr int EIO_LUT_MAX = 16384;           // window entries kept in LDS (64 KiB); the LiTS window has 451

struct SlabArgs {
  const int16_t* vol;
  const int32_t* zsrc;
  const int32_t *y0, *y1, *x0, *x1;
  const float *fy, *fx, *lut;
  float* out;
  int src_d, src_h, src_w, N, H, W, C, lo, hi;
  int total;                                 // N * H * W * C
};

__device__ __forceinline__ int eio_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// one output element by the host's rule, every operation rounded on its own: rows first, then columns
__device__ __forceinline__ float slab_px(const SlabArgs& a, const float* s_lut, int n, int y, int x, int c) {
  const int z = a.zsrc[n * a.C + c];
  if (z < 0 ? z != -2 : z >= a.src_d) return 0.0f;            // -1: a plane of 0.0f (0 * w + 0 * w' is exactly 0)
  float v00, v01, v10, v11;
  if (z == -2) {
    v00 = v01 = v10 = v11 = s_lut[eio_clamp(0, a.lo, a.hi) - a.lo];
  } else {
    const int ya = eio_clamp(a.y0[y], 0, a.src_h - 1), yb = eio_clamp(a.y1[y], 0, a.src_h - 1);
    const int xa = eio_clamp(a.x0[x], 0, a.src_w - 1), xb = eio_clamp(a.x1[x], 0, a.src_w - 1);
    const int16_t* ra = a.vol + (z * a.src_h + ya) * a.src_w;
    const int16_t* rb = a.vol + (z * a.src_h + yb) * a.src_w;
    v00 = s_lut[eio_clamp(ra[xa], a.lo, a.hi) - a.lo];
    v01 = s_lut[eio_clamp(ra[xb], a.lo, a.hi) - a.lo];
    v10 = s_lut[eio_clamp(rb[xa], a.lo, a.hi) - a.lo];
    v11 = s_lut[eio_clamp(rb[xb], a.lo, a.hi) - a.lo];
  }
  const float fy = a.fy[y], fx = a.fx[x];
  const float gy = 1.0f - fy, gx = 1.0f - fx;
  const float r0 = v00 * gy + v10 * fy;
  const float r1 = v01 * gy + v11 * fy;
  return r0 * gx + r1 * fx;
}

// the coordinates of the next element of the flat [N, H, W, C] output
__device__ __forceinline__ void slab_next(const SlabArgs& a, int& n, int& y, int& x, int& c) {
  if (++c < a.C) return;
  c = 0;
  if (++x < a.W) return;
  x = 0;
  if (++y < a.H) return;
  y = 0;
  ++n;
}

template <int V>
__global__ __launch_bounds__(EIO_BLOCK) void eval_slab_kernel(SlabArgs a) {
  extern __shared__ float s_lut[];
  for (int i = threadIdx.x; i <= a.hi - a.lo; i += EIO_BLOCK) s_lut[i] = a.lut[i];
  __syncthreads();
  const int groups = a.total / V;
#pragma unroll 1
  for (int it = 0; it < EIO_ITERS; ++it) {
    const unsigned g = (blockIdx.x * EIO_ITERS + it) * EIO_BLOCK + threadIdx.x;   // unsigned: may pass 2^31 past the end
    if (g > (unsigned)groups) return;
    const int e = (int)g * V;
    const int count = g < (unsigned)groups ? V : a.total - e;  // g == groups: the elements past the last whole group
    if (count <= 0) return;
    unsigned t = (unsigned)e;
    int c = (int)(t % (unsigned)a.C);
    t /= (unsigned)a.C;
    int x = (int)(t % (unsigned)a.W);
    t /= (unsigned)a.W;
    int y = (int)(t % (unsigned)a.H);
    int n = (int)(t / (unsigned)a.H);
    if (count == V) {
      float v[V];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        v[k] = slab_px(a, s_lut, n, y, x, c);
        slab_next(a, n, y, x, c);
      }
      if (V == 4) {
        stg4(a.out + e, make_float4(v[0], v[1 % V], v[2 % V], v[3 % V]));
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) a.out[e + k] = v[k];
      }
    } else {
      for (int k = 0; k < count; ++k) {
        a.out[e + k] = slab_px(a, s_lut, n, y, x, c);
        slab_next(a, n, y, x, c);
      }
    }
  }
}

struct ZoomArgs {
  const uint8_t* src;
  const int32_t *tz, *ty, *tx;
  uint8_t* dst;
  int d, h, w, D, H, W;
  int total;                                 // D * H * W
};

// first source index of output row (z, y), or -1 when either table sends the row outside
__device__ __forceinline__ int zoom_row(const ZoomArgs& a, int z, int y) {
  const int sz = a.tz[z], sy = a.ty[y];
  if ((unsigned)sz >= (unsigned)a.d || (unsigned)sy >= (unsigned)a.h) return -1;
  return (sz * a.h + sy) * a.w;
}

__device__ __forceinline__ uint32_t zoom_px(const ZoomArgs& a, int row, int x) {
  const int sx = a.tx[x];
  return row >= 0 && (unsigned)sx < (unsigned)a.w ? a.src[row + sx] : 0u;
}

// the next voxel of the flat [D, H, W] output; never called past the last voxel (the tables end there)
__device__ __forceinline__ void zoom_next(const ZoomArgs& a, int& z, int& y, int& x, int& row) {
  if (++x < a.W) return;
  x = 0;
  if (++y == a.H) {
    y = 0;
    ++z;
  }
  row = zoom_row(a, z, y);
}

template <int V>
__global__ __launch_bounds__(EIO_BLOCK) void zoom_nearest3d_kernel(ZoomArgs a) {
  const int groups = a.total / V;
  const unsigned g = blockIdx.x * EIO_BLOCK + threadIdx.x;
  if (g > (unsigned)groups) return;
  const int e = (int)g * V;
  const int count = g < (unsigned)groups ? V : a.total - e;
  if (count <= 0) return;
  unsigned t = (unsigned)e;
  int x = (int)(t % (unsigned)a.W);
  t /= (unsigned)a.W;
  int y = (int)(t % (unsigned)a.H);
  int z = (int)(t / (unsigned)a.H);
  int row = zoom_row(a, z, y);
  if (count == V) {
    uint32_t word[(V + 3) / 4] = {};
#pragma unroll
    for (int k = 0; k < V; ++k) {
      word[k / 4] |= zoom_px(a, row, x) << (8 * (k % 4));
      if (k + 1 < V) zoom_next(a, z, y, x, row);
    }
    if (V == 16) {
      constexpr int NW = (V + 3) / 4;
      *reinterpret_cast<uint4*>(a.dst + e) = make_uint4(word[0], word[1 % NW], word[2 % NW], word[3 % NW]);
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) a.dst[e + k] = (uint8_t)(word[k / 4] >> (8 * (k % 4)));
    }
  } else {
    for (int k = 0; k < count; ++k) {
      a.dst[e + k] = (uint8_t)zoom_px(a, row, x);
      if (k + 1 < count) zoom_next(a, z, y, x, row);
    }
  }
}

static inline bool eio_fits(int a, int b, int c, int d = 1) {
  return a > 0 && b > 0 && c > 0 && d > 0 && (int64_t)a * b * c < ((int64_t)1 << 31) &&
         (int64_t)a * b * c * d < ((int64_t)1 << 31);
}

}  // namespace

extern "C" int unetk_eval_slab(const int16_t* vol, int src_d, int src_h, int src_w, const int32_t* zsrc, int N, int C,
                               const int32_t* y0, const int32_t* y1, const float* fy, int H, const int32_t* x0,
                               const int32_t* x1, const float* fx, int W, const float* lut, int lut_n, int lo, int hi,
                               float* images, void* stream) {
  UNETK_REQUIRE(eio_fits(src_d, src_h, src_w) && eio_fits(H, W, C, N));
  UNETK_REQUIRE(hi >= lo && (int64_t)hi - lo + 1 <= (int64_t)lut_n && lo >= -32768 && hi <= 32767);
  UNETK_REQUIRE(vol && zsrc && y0 && y1 && fy && x0 && x1 && fx && lut && images && (((uintptr_t)images) & 3u) == 0);
  if (hi - lo + 1 > EIO_LUT_MAX) return UNETK_E_UNSUPPORTED;
  SlabArgs a;
  a.vol = vol; a.zsrc = zsrc; a.y0 = y0; a.y1 = y1; a.x0 = x0; a.x1 = x1; a.fy = fy; a.fx = fx; a.lut = lut; a.out = images;
  a.src_d = src_d; a.src_h = src_h; a.src_w = src_w; a.N = N; a.H = H; a.W = W; a.C = C; a.lo = lo; a.hi = hi;
  a.total = N * H * W * C;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)(hi - lo + 1) * sizeof(float);
  const int per_block = EIO_BLOCK * EIO_ITERS;
  if (unetk_aligned16(images)) {
    const int groups = a.total / 4 + 1;                        // + 1: the thread that stores the elements past the last group
    UNETK_LAUNCH(eval_slab_kernel<4>, dim3((groups + per_block - 1) / per_block), dim3(EIO_BLOCK), lds, st, a);
  } else {
    UNETK_LAUNCH(eval_slab_kernel<1>, dim3((a.total + per_block - 1) / per_block), dim3(EIO_BLOCK), lds, st, a);
  }
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_zoom_nearest3d(const uint8_t* src, int d, int h, int w, const int32_t* tz, const int32_t* ty,
                                    const int32_t* tx, int D, int H, int W, uint8_t* dst, void* stream) {
  UNETK_REQUIRE(eio_fits(d, h, w) && eio_fits(D, H, W));
  UNETK_REQUIRE(src && tz && ty && tx && dst);
  ZoomArgs a;
  a.src = src; a.tz = tz; a.ty = ty; a.tx = tx; a.dst = dst;
  a.d = d; a.h = h; a.w = w; a.D = D; a.H = H; a.W = W;
  a.total = D * H * W;
  hipStream_t st = (hipStream_t)stream;
  if (unetk_aligned16(dst)) {
    const int groups = a.total / 16 + 1;
    UNETK_LAUNCH(zoom_nearest3d_kernel<16>, dim3((groups + EIO_BLOCK - 1) / EIO_BLOCK), dim3(EIO_BLOCK), 0, st, a);
  } else {
    UNETK_LAUNCH(zoom_nearest3d_kernel<1>, dim3((a.total + EIO_BLOCK - 1) / EIO_BLOCK), dim3(EIO_BLOCK), 0, st, a);
  }
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}
