// `boundary` loss-weight map (loss_metrics.py:149-165), entirely on the device.
//
// The reference builds it per step through a HOST round trip: one-hot -> 3x3 dilation ring per class -> tf.py_func
// (scipy.ndimage.distance_transform_edt) -> exp(-d/25) + 1 -> per-sample normalisation to mean 1.  Here:
//   ring(p)   = some in-bounds 3x3 neighbour carries a label different from p's   (== sum_c (dilate(onehot_c) - onehot_c) > 0)
//   g(h, w)   = row distance from (h, w) to the nearest ring pixel of column w     (two scans per column)
//   d2(h, w)  = min_w' (w - w')^2 + g(h, w')^2                                     (exact squared Euclidean distance)
//   d         = (float) sqrt((double) d2)      -- what scipy returns after .astype(float32): bit-exact
//   w         = exp(-d / 25) + 1, then w * H*W / sum_hw(w) with a fixed-order sum (bit-reproducible)
// An image without any ring pixel (a single label) has no zero for the EDT to measure to; scipy (1.15) then returns
// sqrt((h+1)^2 + w^2), which is reproduced so that such slices weigh as they do in the reference.
// HBM-bound and tiny next to the network (one int32 read + a few float passes over [N,H,W]).
#include "common.h"
#include "edt_int.h"

namespace {

constexpr int G_INF = 1 << 20;

// thread = (n, w) column: ring detection + downward / upward scans
__global__ __launch_bounds__(256) void edt_columns_kernel(const int32_t* __restrict__ lab, int N, int H, int W,
                                                          int32_t* __restrict__ g, int32_t* __restrict__ has_ring) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * W) return;
  const int n = i / W, w = i - n * W;
  const int32_t* L = lab + (int64_t)n * H * W;
  int32_t* G = g + (int64_t)n * H * W;
  int last = -G_INF;
  bool any = false;
  for (int h = 0; h < H; ++h) {
    const int32_t own = L[(int64_t)h * W + w];
    bool ring = false;
    for (int dh = -1; dh <= 1; ++dh) {
      const int hh = h + dh;
      if (hh < 0 || hh >= H) continue;
      for (int dw = -1; dw <= 1; ++dw) {
        const int ww = w + dw;
        if (ww < 0 || ww >= W) continue;
        ring |= L[(int64_t)hh * W + ww] != own;
      }
    }
    if (ring) { last = h; any = true; }
    G[(int64_t)h * W + w] = min(h - last, G_INF);
  }
  last = G_INF * 2;
  for (int h = H - 1; h >= 0; --h) {
    const int64_t o = (int64_t)h * W + w;
    if (G[o] == 0) last = h;
    G[o] = min(G[o], min(last - h, G_INF));
  }
  if (any) atomicOr(&has_ring[n], 1);
}

// block = one image row (n, h); the row of g sits in LDS; thread = output column(s)
__global__ __launch_bounds__(256) void edt_rows_kernel(const int32_t* __restrict__ g, const int32_t* __restrict__ has_ring,
                                                       int N, int H, int W, float* __restrict__ wmap,
                                                       float* __restrict__ row_sums) {
  extern __shared__ int32_t grow[];
  __shared__ float red[256];
  const int row = blockIdx.x;
  const int n = row / H, h = row - n * H;
  const int32_t* G = g + (int64_t)row * W;
  for (int w = threadIdx.x; w < W; w += 256) grow[w] = G[w];
  __syncthreads();
  const bool ring = has_ring[n] != 0;
  float part = 0.f;
  for (int w = threadIdx.x; w < W; w += 256) {
    int64_t d2;
    if (ring) {
      d2 = (int64_t)1 << 60;
      for (int k = 0; k < W; ++k) {
        const int64_t gv = grow[k];
        if (gv >= G_INF) continue;
        const int64_t dx = w - k;
        d2 = min(d2, dx * dx + gv * gv);
      }
    } else {
      d2 = (int64_t)(h + 1) * (h + 1) + (int64_t)w * w;
    }
    const float d = (float)sqrt((double)d2);
    const float v = expf(-d / 25.f) + 1.f;
    wmap[(int64_t)row * W + w] = v;
    part += v;
  }
  red[threadIdx.x] = part;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) row_sums[row] = red[0];
}

__global__ __launch_bounds__(256) void edt_normalise_kernel(float* __restrict__ wmap, const float* __restrict__ row_sums,
                                                            int N, int H, int W) {
  const int n = blockIdx.y;
  double s = 0.0;
  for (int h = 0; h < H; ++h) s += (double)row_sums[n * H + h];          // fixed order, every thread the same value
  const float scale = (float)((double)H * (double)W / s);
  float* M = wmap + (int64_t)n * H * W;
  const int64_t total = (int64_t)H * W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
    M[i] *= scale;
}


// ------------------------------------------------------------------------------------------------ 3-D
// The same map over a label PATCH [N, D, H, W] with an integer z scale K (include/unetk.h has the full statement): the ring is the
// 3x3x3 one, d2 = min over ring voxels of (K dz)^2 + dy^2 + dx^2.  Three separable passes over int32 fields:
//   b3_x_kernel          a wave per line (n, z, y): ring detection, one bit per voxel in LDS, 64 voxels per ballot; every voxel finds the
//                        nearest set bit of its line (edt_int.h) -> g1 = gx^2, or IEDT_NONE on a line without a ring voxel
//   b3_axis_kernel<0>    y: g2(y) = min over y' of (y - y')^2 + g1(y'), brute force over a 64-column strip (edt_int.h)
//   b3_axis_kernel<1>    z: d2(z) = min over z' of K^2 (z - z')^2 + g2(z'), the same loop along the other axis, then sqrt / expf and a
//                        block's sum of the weights in double, tree-reduced in a fixed order
//   b3_normalise_kernel  every block adds the sample's block sums in the same order, then scales its share of the map
// A sample without a ring voxel keeps IEDT_NONE through every minimum: its voxels get w = 1 and d2 = -1, with no flag to consult.
// Integer arithmetic up to the sqrt, no atomics: two calls give identical bits.
constexpr int B3_MAX_D = 1024, B3_MAX_HW = IEDT_MAX_BITS, B3_MAX_K = 16;
static_assert(iedt_fits(1, B3_MAX_HW) && iedt_fits(B3_MAX_K * B3_MAX_K, B3_MAX_D), "b3_axis_kernel overflows int32");
static_assert((int64_t)B3_MAX_K * B3_MAX_K * (B3_MAX_D - 1) * (B3_MAX_D - 1) + 2 * (int64_t)(B3_MAX_HW - 1) * (B3_MAX_HW - 1) < IEDT_NONE,
              "a real d2 reaches the sentinel");
constexpr int B3_LINES = 4;               // lines of a block of b3_x_kernel: one per wave

// the sum of the block's 256 `part`s, paired s = 128, 64, .., 1: the order is part of the map's bits
__device__ __forceinline__ double b3_block_sum(double part) {
  __shared__ double red[256];
  red[threadIdx.x] = part;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(256) void b3_x_kernel(const int32_t* __restrict__ lab, int D, int H, int W, int64_t lines,
                                                   int32_t* __restrict__ g1) {
  __shared__ unsigned long long bits[B3_LINES][B3_MAX_HW / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t line = (int64_t)blockIdx.x * B3_LINES + wave;   // (n * D + z) * H + y
  const bool live = line < lines;                               // wave-uniform
  const int64_t l = live ? line : 0;
  const int y = (int)(l % H), z = (int)((l / H) % D);
  const int64_t plane = (int64_t)H * W;
  // the nine rows of the neighbourhood; one outside the SAMPLE's volume is replaced by the nearest one inside, which is a row of
  // the neighbourhood too (a neighbour that changes nothing)
  const int32_t* row = lab + l * W;
  const int32_t* nb[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int cz = min(max(z + k / 3 - 1, 0), D - 1), cy = min(max(y + k % 3 - 1, 0), H - 1);
    nb[k] = row + (int64_t)(cz - z) * plane + (int64_t)(cy - y) * W;
  }
  for (int x0 = 0; x0 < W; x0 += 64) {                          // block-uniform trip count: the ballots see whole waves
    const int x = x0 + lane;
    bool ring = false;
    if (live && x < W) {
      const int32_t own = row[x];
      const int xl = max(x - 1, 0), xr = min(x + 1, W - 1);
#pragma unroll
      for (int k = 0; k < 9; ++k) ring |= nb[k][xl] != own || nb[k][x] != own || nb[k][xr] != own;
    }
    const unsigned long long w = __ballot(ring);
    if (lane == 0) bits[wave][x0 >> 6] = w;
  }
  __syncthreads();
  if (!live) return;
  const unsigned long long* b = bits[wave];
  const int nwords = (W + 63) >> 6;
  int32_t* o = g1 + l * W;
  for (int x = lane; x < W; x += 64) {
    const int g = iedt_nearest_bit(b, nwords, x);
    o[x] = g < 0 ? IEDT_NONE : g * g;
  }
}

// out(i) = min over j of scale * (i - j)^2 + in(j) along one axis of length L and element stride `stride`, for the W columns of a
// slab (consecutive in memory).  Slab s starts at (s / sps) * sample + (s % sps) * slab_stride: the y pass walks the planes of a
// sample (sps = D, slab_stride = H * W, stride = W), the z pass its rows (sps = H, slab_stride = W, stride = H * W).  No slab
// spans two samples, so no sample sees another's ring.
template <bool FINAL>
__global__ __launch_bounds__(256) void b3_axis_kernel(const int32_t* __restrict__ in, int L, int64_t stride, int W, int nxb, int sps,
                                                      int64_t sample, int64_t slab_stride, int scale, int32_t* __restrict__ out,
                                                      float* __restrict__ wmap, int32_t* __restrict__ d2_out,
                                                      double* __restrict__ block_sums) {
  __shared__ int stage[IEDT_STAGE][64];
  const int slab = blockIdx.x / nxb, xb = (blockIdx.x - slab * nxb) * 64, t0 = blockIdx.y * IEDT_T;
  const int n = slab / sps;
  const int64_t base = (int64_t)n * sample + (int64_t)(slab - n * sps) * slab_stride;
  const int x = xb + (threadIdx.x & 63), i0 = t0 + (threadIdx.x >> 6) * 4;   // the thread's outputs: i0 .. i0 + 3 along the axis, column x
  int best[4];
  iedt_axis_min(stage, in + base + x, x < W, stride, L, i0, scale, best);
  if (!FINAL) {
    if (x >= W) return;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i0 + k < L) out[base + (int64_t)(i0 + k) * stride + x] = best[k];
    return;
  }
  double part = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (x >= W || i0 + k >= L) continue;
    const int64_t o = base + (int64_t)(i0 + k) * stride + x;
    const bool has = best[k] < IEDT_NONE;
    float v = 1.f;
    if (has) {
      const float d = (float)sqrt((double)best[k]);
      v = expf(-d / 25.f) + 1.f;
    }
    wmap[o] = v;
    if (d2_out) d2_out[o] = has ? best[k] : -1;
    part += (double)v;
  }
  const double sum = b3_block_sum(part);
  // the sample's sums are consecutive: [n][blockIdx.y][the sample's share of blockIdx.x]
  const int per = sps * nxb;
  if (threadIdx.x == 0) block_sums[((int64_t)n * gridDim.y + blockIdx.y) * per + (blockIdx.x - n * per)] = sum;
}

__global__ __launch_bounds__(256) void b3_normalise_kernel(float* __restrict__ wmap, const double* __restrict__ block_sums, int per_sample,
                                                           int64_t vox) {
  const int n = blockIdx.y;
  double s = 0.0;
  for (int i = threadIdx.x; i < per_sample; i += 256) s += block_sums[(int64_t)n * per_sample + i];   // the same order in every block
  const float scale = (float)((double)vox / b3_block_sum(s));
  float* M = wmap + (int64_t)n * vox;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < vox; i += (int64_t)gridDim.x * blockDim.x) M[i] *= scale;
}

bool b3_valid(int N, int D, int H, int W) { return N > 0 && N <= 65535 && D > 0 && H > 0 && W > 0; }
bool b3_supported(int N, int D, int H, int W) {
  if (D > B3_MAX_D || H > B3_MAX_HW || W > B3_MAX_HW) return false;
  // every launch's grid.x: lines / 4, planes x strips, rows x strips
  return (int64_t)N * D * H * ((W + 63) / 64) < ((int64_t)1 << 31);
}
int64_t b3_sums_per_sample(int D, int H, int W) { return (int64_t)H * ((W + 63) / 64) * ((D + IEDT_T - 1) / IEDT_T); }

}  // namespace

extern "C" size_t unetk_boundary_weights_ws_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return ((size_t)N * H * W + (size_t)N * H + (size_t)N + 64) * 4;
}

extern "C" int unetk_boundary_weights(const int32_t* labels, int N, int H, int W, float* wmap, void* ws, size_t ws_bytes,
                                      void* stream) {
  UNETK_REQUIRE(labels && wmap && ws && N > 0 && H > 0 && W > 0);
  if (W > 12 * 1024 || H >= G_INF) return UNETK_E_UNSUPPORTED;
  if (ws_bytes < unetk_boundary_weights_ws_bytes(N, H, W)) return UNETK_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int32_t* g = (int32_t*)ws;
  float* row_sums = (float*)(g + (size_t)N * H * W);
  int32_t* has_ring = (int32_t*)(row_sums + (size_t)N * H);
  hipError_t e = hipMemsetAsync(has_ring, 0, (size_t)N * 4, st);
  if (e != hipSuccess) return (int)e;
  UNETK_LAUNCH(edt_columns_kernel, dim3((N * W + 255) / 256), dim3(256), 0, st, labels, N, H, W, g, has_ring);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(edt_rows_kernel, dim3(N * H), dim3(256), (size_t)W * 4, st, g, has_ring, N, H, W, wmap, row_sums);
  UNETK_LAUNCH_CHECK();
  const int gx = (int)min((int64_t)1024, ((int64_t)H * W + 255) / 256);
  UNETK_LAUNCH(edt_normalise_kernel, dim3(gx, N), dim3(256), 0, st, wmap, row_sums, N, H, W);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" size_t unetk_boundary_weights3d_ws_bytes(int N, int D, int H, int W) {
  if (!b3_valid(N, D, H, W) || !b3_supported(N, D, H, W)) return 0;
  return (size_t)N * b3_sums_per_sample(D, H, W) * sizeof(double) + (size_t)N * D * H * W * sizeof(int32_t);
}

extern "C" int unetk_boundary_weights3d(const int32_t* labels, int N, int D, int H, int W, int z_scale, float* wmap, int32_t* d2_out,
                                        void* ws, size_t ws_bytes, void* stream) {
  UNETK_REQUIRE(labels && wmap && ws && b3_valid(N, D, H, W));
  UNETK_REQUIRE(((((uintptr_t)labels) | ((uintptr_t)wmap) | ((uintptr_t)d2_out)) & 3u) == 0 && unetk_aligned16(ws));
  if (z_scale < 1 || z_scale > B3_MAX_K || !b3_supported(N, D, H, W)) return UNETK_E_UNSUPPORTED;
  if (ws_bytes < unetk_boundary_weights3d_ws_bytes(N, D, H, W)) return UNETK_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int per = (int)b3_sums_per_sample(D, H, W), nxb = (W + 63) / 64;
  const int64_t plane = (int64_t)H * W, vox = plane * D, lines = (int64_t)N * D * H;
  double* block_sums = static_cast<double*>(ws);
  int32_t* g2 = reinterpret_cast<int32_t*>(block_sums + (size_t)N * per);
  int32_t* g1 = reinterpret_cast<int32_t*>(wmap);               // the map's own storage holds the x pass until the z pass writes it
  UNETK_LAUNCH(b3_x_kernel, dim3((unsigned)((lines + B3_LINES - 1) / B3_LINES)), dim3(256), 0, st, labels, D, H, W, lines, g1);
  UNETK_LAUNCH(b3_axis_kernel<false>, dim3((unsigned)(N * D * nxb), (H + IEDT_T - 1) / IEDT_T), dim3(256), 0, st, (const int32_t*)g1, H,
               (int64_t)W, W, nxb, D, vox, plane, 1, g2, (float*)nullptr, (int32_t*)nullptr, (double*)nullptr);
  UNETK_LAUNCH(b3_axis_kernel<true>, dim3((unsigned)(N * H * nxb), (D + IEDT_T - 1) / IEDT_T), dim3(256), 0, st, (const int32_t*)g2, D,
               plane, W, nxb, H, vox, (int64_t)W, z_scale * z_scale, (int32_t*)nullptr, wmap, d2_out, block_sums);
  const int gx = (int)min((int64_t)1024, (vox + 255) / 256);
  UNETK_LAUNCH(b3_normalise_kernel, dim3(gx, N), dim3(256), 0, st, wmap, (const double*)block_sums, per, vox);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}
