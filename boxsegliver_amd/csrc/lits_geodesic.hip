// Geodesic click guides for the click-guided 2-D batches (--geodesic_guide; DESIGN.md 7.3.7.1, definition in include/unetk.h).
//
// The reference grows the geodesic distance from the clicks on the half-resolution centre channel with GeodisTK's fast
// marching on the host (DataLoader/NF/input_pipeline_g_simply.py:471-496, entry/main_eval.py:205-220).  Here the distance is
// DEFINED as the float32 shortest path on the 8-connected grid, whose fixed point does not depend on the relaxation order:
//   unetk_lits_inter_center  the base field I = pixel (2i, 2j) of channel C / 2 of unetk_lits_inter_batch (training = 0, no
//                            flips), from the same moments and the same per-pixel expression (lits_inter_px.h)
//   unetk_click_geodesic     geo_solve_kernel  one workgroup per (sample, kind), start to convergence inside one launch
//                            geo_guide_kernel  resize_bilinear(align_corners) of both kinds' D to H x W through the row's flips
//
// The solve.  I and D live with a one-pixel halo (D = +inf, I = 0 there: a halo neighbour offers +inf and never wins), in LDS
// (path 1) or in the workspace (path 2).  A sweep relaxes every pixel IN PLACE: thread t owns the pixels t, t + 1024, ... in
// row-major order, reads the 8 neighbours' D as they are at that moment and lowers its own D to the best offer.  D only ever
// decreases and every value it takes is the float32 length of a real path, so a stale read costs a sweep, never a bit; a
// sweep in which nobody lowered anything has seen a constant D that satisfies the fixed-point equation everywhere, and ends
// the loop.  Dword reads and writes do not tear.  The loop is bounded at hh * hw sweeps (Bellman-Ford); reaching the bound
// sets status bit 8.  Before the eight square roots a pixel tests fl(min neighbour + 1) < D: c >= 1 and float addition is
// monotone, so no offer can beat that, and the pixels ahead of the front cost eight reads.  (Skipping every pixel whose
// neighbours are unchanged since its last evaluation -- an exact test on the sum of their bit patterns -- was built and
// measured SLOWER, 2.44 against 1.56 ms at batch 16: behind the front the values keep settling for many sweeps, and the
// second pass over the changed pixels diverges.  DESIGN.md 7.3.7.1.)
//
// LDS pitch (path 1): a 32-lane half of ds_read_b32 conflicts on (address / 4) % 32.  The half's pixels are 32 consecutive
// row-major indices, at word address index + row * (pitch - hw) + const: with pitch - hw = 32 they are 32 distinct banks for
// every hw and every one of the 8 shifted reads; with hw % 32 == 0 a half never leaves its row and pitch - hw = 2 does the
// same in less room (128 x 128: 2 * 130 * 130 words of the 160 KiB).  Where 32 does not fit, 2 is used and a half that
// straddles a row end pays two lanes.
#include "common.h"
#include "lits_geom.h"
#include "lits_inter_px.h"
#include "lits_patch.h"

// every operation of the definition rounds on its own (unetk.h): what follows is compiled without contraction; the shared
// headers above keep the contraction unetk_lits_inter_batch is built with, so the base field has its bits
#pragma clang fp contract(off)

namespace {

constexpr int GEO_THREADS = 1024;
constexpr int GEO_MAX_GRID = 1 << 18;            // hh * hw of path 2
constexpr int GEO_LDS_BYTES = 160 * 1024 - 1024; // dynamic LDS of path 1; the rest holds the seeds and the flags
constexpr int GEO_MAXK = UNETK_INTER_MAX_CLICKS;

struct GeoGrid {
  int hh, hw, pitch, path;                       // pitch of the haloed fields; path 0 unsupported, 1 LDS, 2 workspace
};
inline size_t geo_field_words(const GeoGrid& g) { return (size_t)(g.hh + 2) * g.pitch; }
GeoGrid geo_grid(const unetk_lits_inter_desc* d) {
  GeoGrid g;
  g.hh = (d->H + 1) / 2;
  g.hw = (d->W + 1) / 2;
  g.pitch = g.hw + 2;
  g.path = 0;
  if ((int64_t)g.hh * g.hw > GEO_MAX_GRID || (int64_t)d->H * d->W >= ((int64_t)1 << 31)) return g;
  const int wide = g.hw + 32;
  if (g.hw % 32 != 0 && (size_t)(g.hh + 2) * wide * 2 * sizeof(float) <= (size_t)GEO_LDS_BYTES) g.pitch = wide;
  g.path = geo_field_words(g) * 2 * sizeof(float) <= (size_t)GEO_LDS_BYTES ? 1 : 2;
  if (g.path == 2) g.pitch = g.hw + 2;
  return g;
}
inline size_t geo_round16(size_t v) { return (v + 15) / 16 * 16; }

// ------------------------------------------------------------------------------------------------ base field
__global__ __launch_bounds__(256) void geo_center_kernel(unetk_lits_inter_desc d, int hh, int hw,
                                                         const uint16_t* __restrict__ slices, const int32_t* __restrict__ tab,
                                                         const float* __restrict__ stat, float* __restrict__ base,
                                                         int32_t* __restrict__ status) {
  const int n = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const Box2 b = ib_box(tab + (int64_t)n * TW, d);
  const int64_t sl = ib_slice(b, 0, d);
  if (sl < 0 && i == 0) atomicOr(status, 2);
  if (i >= hh * hw) return;
  const int gy = i / hw, gx = i - gy * hw;
  float v = 0.f;
  if (sl >= 0) {
    const float m = stat[(int64_t)n * ST_N + ST_M], den = stat[(int64_t)n * ST_N + ST_S] + 1e-8f;
    const float hs = lits_ac_scale(b.ch, d.H), ws = lits_ac_scale(b.cw, d.W);
    const int64_t plane = (int64_t)d.src_h * d.src_w;
    const IbTaps tp = ib_taps(2 * gy, 2 * gx, b, hs, ws);
    v = ib_value(slices + sl * plane + (int64_t)b.y1 * d.src_w + b.x1, d.src_w, tp, (float)d.im_scale, m, den);
  }
  base[(int64_t)n * hh * hw + i] = v;
}

// ------------------------------------------------------------------------------------------------ seeds
// input_pipeline_g_simply.py:483: (int)(y / ch * H / 2) in float32, each operation rounded, truncated toward zero, clamped
// into the grid (the clamp comes first here: it is the same for every value an int holds and never converts a float that an
// int cannot hold)
__device__ __forceinline__ int geo_seed(int y, int ch, int H, int extent) {
  const float r = (float)y / (float)ch;
  const float s = r * (float)H;
  const float g = s / 2.0f;
  return (int)fminf(fmaxf(g, 0.f), (float)(extent - 1));
}

// ------------------------------------------------------------------------------------------------ the solve
__device__ __forceinline__ float geo_offer(float dp, float ip, float iq, float s2) {
  const float di = ip - iq;
  const float sq = di * di;
  const float c = sqrtf(s2 + sq);
  return dp + c;
}
// one pixel at word `a` of the haloed fields; returns whether its D was lowered
__device__ __forceinline__ bool geo_relax(const float* I, float* D, int a, int pitch) {
  const float d0 = D[a - pitch - 1], d1 = D[a - pitch], d2 = D[a - pitch + 1], d3 = D[a - 1];
  const float d4 = D[a + 1], d5 = D[a + pitch - 1], d6 = D[a + pitch], d7 = D[a + pitch + 1];
  const float dq = D[a];
  const float mn = fminf(fminf(fminf(d0, d1), fminf(d2, d3)), fminf(fminf(d4, d5), fminf(d6, d7)));
  if (!(mn + 1.0f < dq)) return false;
  const float iq = I[a];
  float best = geo_offer(d0, I[a - pitch - 1], iq, 2.0f);
  best = fminf(best, geo_offer(d1, I[a - pitch], iq, 1.0f));
  best = fminf(best, geo_offer(d2, I[a - pitch + 1], iq, 2.0f));
  best = fminf(best, geo_offer(d3, I[a - 1], iq, 1.0f));
  best = fminf(best, geo_offer(d4, I[a + 1], iq, 1.0f));
  best = fminf(best, geo_offer(d5, I[a + pitch - 1], iq, 2.0f));
  best = fminf(best, geo_offer(d6, I[a + pitch], iq, 1.0f));
  best = fminf(best, geo_offer(d7, I[a + pitch + 1], iq, 2.0f));
  if (best < dq) {
    D[a] = best;
    return true;
  }
  return false;
}

// grid (2, N): block (kind, n).  out f32 [N][2][hh][hw]; sweeps int32 [N][2]; fields: path 2's haloed I and D per block.
template <bool LDS>
__global__ __launch_bounds__(GEO_THREADS) void geo_solve_kernel(unetk_lits_inter_desc d, int hh, int hw, int pitch,
                                                                 const int32_t* __restrict__ tab, const float* __restrict__ base,
                                                                 const int32_t* __restrict__ pts, const int32_t* __restrict__ cnt,
                                                                 int K, float* __restrict__ out, int32_t* __restrict__ sweeps,
                                                                 float* __restrict__ fields, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) float geo_smem[];
  __shared__ int seed_at[GEO_MAXK];
  __shared__ int flag[3];
  const int kind = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const int total = hh * hw;
  const int64_t pair = (int64_t)n * 2 + kind;
  float* dst = out + pair * total;
  const int k = min(max(cnt[pair], 0), K);
  if (k == 0) {                                              // block-uniform: false_fn, exactly 0
    for (int i = tid; i < total; i += GEO_THREADS) dst[i] = 0.f;
    if (tid == 0) sweeps[pair] = 0;
    return;
  }
  const int words = (hh + 2) * pitch;
  float* I = LDS ? geo_smem : fields + pair * 2 * (int64_t)words;
  float* D = I + words;
  const float* src = base + (int64_t)n * total;
  for (int i = tid; i < words; i += GEO_THREADS) {
    const int y = i / pitch - 1, x = i - (y + 1) * pitch - 1;
    const bool in = y >= 0 && y < hh && x >= 0 && x < hw;
    I[i] = in ? src[y * hw + x] : 0.f;
    D[i] = INFINITY;
  }
  if (tid < k) {
    const Box2 b = ib_box(tab + (int64_t)n * TW, d);
    const int32_t* p = pts + (pair * K + tid) * 2;
    seed_at[tid] = (geo_seed(p[0], b.ch, d.H, hh) + 1) * pitch + geo_seed(p[1], b.cw, d.W, hw) + 1;
  }
  if (tid < 3) flag[tid] = 0;
  __syncthreads();
  if (tid < k) D[seed_at[tid]] = 0.f;
  __syncthreads();

  // thread t owns pixels t, t + 1024, ...: (y, x) advance without a division
  const int step_y = GEO_THREADS / hw, step_x = GEO_THREADS - step_y * hw;
  const int y_first = tid / hw, x_first = tid - y_first * hw;
  int done = 0;
  bool converged = false;
  for (int s = 0; s < total; ++s) {                          // Bellman-Ford: no order needs more sweeps than pixels
    const int cur = s % 3;
    if (tid == 0) flag[(s + 1) % 3] = 0;                     // read last in sweep s - 2, written next in sweep s + 1
    bool changed = false;
    int y = y_first, x = x_first;
    for (int i = tid; i < total; i += GEO_THREADS) {
      changed |= geo_relax(I, D, (y + 1) * pitch + x + 1, pitch);
      x += step_x;
      y += step_y;
      if (x >= hw) {
        x -= hw;
        ++y;
      }
    }
    if (changed) flag[cur] = 1;
    __syncthreads();
    done = s + 1;
    if (flag[cur] == 0) {                                    // block-uniform
      converged = true;
      break;
    }
  }
  if (tid == 0) {
    sweeps[pair] = done;
    if (!converged) atomicOr(status, 8);
  }
  int y = y_first, x = x_first;
  for (int i = tid; i < total; i += GEO_THREADS) {
    dst[i] = D[(y + 1) * pitch + x + 1];
    x += step_x;
    y += step_y;
    if (x >= hw) {
      x -= hw;
      ++y;
    }
  }
}

// ------------------------------------------------------------------------------------------------ the guide
// resize_bilinear(align_corners) of D [hh, hw] to H x W (:487), written through the row's flips
__global__ __launch_bounds__(256) void geo_guide_kernel(unetk_lits_inter_desc d, int hh, int hw, const int32_t* __restrict__ tab,
                                                        const float* __restrict__ dist, float* __restrict__ guide) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int area = d.H * d.W;
  if (i >= (int64_t)d.N * area) return;
  const int n = (int)(i / area), r = (int)(i - (int64_t)n * area);
  const int y = r / d.W, x = r - y * d.W;
  const int32_t* t = tab + (int64_t)n * TW;
  const LitsTaps ty = lits_ac_taps(y * lits_ac_scale(hh, d.H), hh), tx = lits_ac_taps(x * lits_ac_scale(hw, d.W), hw);
  const int y0 = min(ty.i0, hh - 1), x0 = min(tx.i0, hw - 1);
  float g[2];
#pragma unroll
  for (int kind = 0; kind < 2; ++kind) {
    const float* p = dist + ((int64_t)n * 2 + kind) * hh * hw;
    g[kind] = lits_bilerp(p[y0 * hw + x0], p[y0 * hw + tx.i1], p[ty.i1 * hw + x0], p[ty.i1 * hw + tx.i1], tx.f, ty.f);
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

bool geo_center_supported(const unetk_lits_inter_desc* d) { return ib_supported(d); }

}  // namespace

extern "C" size_t unetk_lits_inter_center_ws_bytes(const unetk_lits_inter_desc* d) {
  if (!ib_valid(d) || !geo_center_supported(d)) return 0;
  return (size_t)d->N * ib_blocks(d) * (3 * sizeof(double) + 2 * sizeof(float)) + (size_t)d->N * ST_N * sizeof(float);
}

extern "C" int unetk_lits_inter_center(const unetk_lits_inter_desc* d, const uint16_t* slices, const int32_t* sample_tab,
                                       float* base, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  UNETK_REQUIRE(ib_valid(d) && slices && sample_tab && base && status && ws);
  UNETK_REQUIRE((((uintptr_t)slices) & 1u) == 0 && ((((uintptr_t)sample_tab) | ((uintptr_t)base) | ((uintptr_t)status)) & 3u) == 0);
  UNETK_REQUIRE(unetk_aligned16(ws));
  if (!geo_center_supported(d)) return UNETK_E_UNSUPPORTED;
  if (ws_bytes < unetk_lits_inter_center_ws_bytes(d)) return UNETK_E_WORKSPACE;
  // the partial blocks of unetk_lits_inter_batch, so that m and s are its bits
  const int P = ib_blocks(d);
  double* part = static_cast<double*>(ws);
  float* minmax = reinterpret_cast<float*>(part + (size_t)d->N * P * 3);
  float* stat = minmax + (size_t)d->N * P * 2;
  const int hh = (d->H + 1) / 2, hw = (d->W + 1) / 2;
  hipStream_t st = (hipStream_t)stream;
  UNETK_LAUNCH(ib_mask_stats_kernel, dim3(P, d->N), dim3(256), 0, st, *d, slices, sample_tab, part);
  UNETK_LAUNCH(p3d_finalize_kernel, dim3(d->N), dim3(64), 0, st, 0, P, (const double*)part, (const float*)minmax, stat);
  UNETK_LAUNCH(geo_center_kernel, dim3((hh * hw + 255) / 256, d->N), dim3(256), 0, st, *d, hh, hw, slices, sample_tab,
               (const float*)stat, base, status);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_click_geodesic_path(const unetk_lits_inter_desc* d) {
  if (!ib_valid(d)) return 0;
  return geo_grid(d).path;
}

// ws: int32 sweeps[N][2] (the sweeps each solve ran, the one that found nothing to lower included; 0 for a kind without
// clicks), then D f32 [N][2][hh][hw] where the caller passes no `dist`, then path 2's haloed fields
extern "C" size_t unetk_click_geodesic_ws_bytes(const unetk_lits_inter_desc* d) {
  if (!ib_valid(d)) return 0;
  const GeoGrid g = geo_grid(d);
  if (g.path == 0) return 0;
  size_t bytes = geo_round16((size_t)d->N * 2 * sizeof(int32_t)) + geo_round16((size_t)d->N * 2 * g.hh * g.hw * sizeof(float));
  if (g.path == 2) bytes += (size_t)d->N * 2 * 2 * geo_field_words(g) * sizeof(float);
  return bytes;
}

extern "C" int unetk_click_geodesic(const unetk_lits_inter_desc* d, const int32_t* sample_tab, const float* base,
                                    const int32_t* pts, const int32_t* cnt, int K, float* guide, float* dist, int32_t* status,
                                    void* ws, size_t ws_bytes, void* stream) {
  UNETK_REQUIRE(ib_valid(d) && sample_tab && base && pts && cnt && guide && status && ws && (d->G == 1 || d->G == 2));
  UNETK_REQUIRE(K >= 1 && K <= GEO_MAXK);
  UNETK_REQUIRE(((((uintptr_t)sample_tab) | ((uintptr_t)base) | ((uintptr_t)pts) | ((uintptr_t)cnt) | ((uintptr_t)guide) |
                  ((uintptr_t)dist) | ((uintptr_t)status)) & 3u) == 0);
  UNETK_REQUIRE(unetk_aligned16(ws));
  const GeoGrid g = geo_grid(d);
  const int64_t total = (int64_t)d->N * d->H * d->W;
  if (g.path == 0 || (total + 255) / 256 >= ((int64_t)1 << 31)) return UNETK_E_UNSUPPORTED;
  if (ws_bytes < unetk_click_geodesic_ws_bytes(d)) return UNETK_E_WORKSPACE;
  uint8_t* w = static_cast<uint8_t*>(ws);
  int32_t* sweeps = reinterpret_cast<int32_t*>(w);
  w += geo_round16((size_t)d->N * 2 * sizeof(int32_t));
  float* own = reinterpret_cast<float*>(w);
  w += geo_round16((size_t)d->N * 2 * g.hh * g.hw * sizeof(float));
  float* fields = reinterpret_cast<float*>(w);
  float* out = dist ? dist : own;
  hipStream_t st = (hipStream_t)stream;
  if (g.path == 1) {
    const size_t lds = geo_field_words(g) * 2 * sizeof(float);
    static size_t attr_bytes = 0;                            // raised only: the attribute is the kernel's, not the launch's
    if (lds > attr_bytes) {
      hipError_t e = hipFuncSetAttribute((const void*)geo_solve_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
      attr_bytes = lds;
    }
    UNETK_LAUNCH(geo_solve_kernel<true>, dim3(2, d->N), dim3(GEO_THREADS), lds, st, *d, g.hh, g.hw, g.pitch, sample_tab, base, pts,
                 cnt, K, out, sweeps, fields, status);
  } else {
    UNETK_LAUNCH(geo_solve_kernel<false>, dim3(2, d->N), dim3(GEO_THREADS), 0, st, *d, g.hh, g.hw, g.pitch, sample_tab, base, pts,
                 cnt, K, out, sweeps, fields, status);
  }
  UNETK_LAUNCH(geo_guide_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, *d, g.hh, g.hw, sample_tab,
               (const float*)out, guide);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}
