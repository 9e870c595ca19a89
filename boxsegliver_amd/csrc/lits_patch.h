// Passes shared by the LiTS patch pipelines that z-score a crop and gamma-augment the result (lits3d.hip: 3-D patches,
// lits_inter.hip: 2-D click-guided batches): the sample table's crop clamp, the 3-D crop box (also lits3d_clicks.hip's), the
// block reductions, the finalising block and the two gamma passes.  One copy, so the pipelines cannot drift; every reduction
// goes through fp64 per-block partials that a finalising block walks by index -- no floating-point atomics, identical bits
// on every call.
//   workspace: double sums[N][P][3], float minmax[N][P][2] (the blocks' partials: see "block reductions"), then
//              float stat[N][8] = {m, s, mn, sd, min, range, new_mn, new_sd}
#pragma once
#include "common.h"

namespace {

constexpr int TW = UNETK_LITS3D_TAB_COLS;
constexpr int P3D_MAX_BLOCKS = 256;      // partial blocks per sample
constexpr int P3D_VOX_PER_BLOCK = 4096;
enum { ST_M = 0, ST_S, ST_MN, ST_SD, ST_MIN, ST_RNG, ST_NMN, ST_NSD, ST_N };

inline int p3d_blocks_for(int64_t vox) {
  const int64_t p = (vox + P3D_VOX_PER_BLOCK - 1) / P3D_VOX_PER_BLOCK;
  return (int)(p < 1 ? 1 : (p > P3D_MAX_BLOCKS ? P3D_MAX_BLOCKS : p));
}

// ------------------------------------------------------------------------------------------------ 3-D crop box
// The box of one sample-table row, for every descriptor that carries D, src_h, src_w and n_slices (unetk_lits3d_desc,
// unetk_lits3d_clicks_desc): patches, window accumulation and the 3-D click simulator cut the same voxels.
struct Box3 {
  int64_t base;
  int depth, z1, y1, x1, ch, cw;
};
// DataLoader/misc.py:132-143 volume_crop, with the crop clamped to the slice and a case shallower than D starting at 0
template <class Desc>
__device__ __forceinline__ Box3 p3d_box(const int32_t* __restrict__ t, const Desc& d) {
  Box3 b;
  b.base = t[0];
  b.depth = max(t[1], 0);
  b.ch = min(max(t[5], 1), d.src_h);
  b.cw = min(max(t[6], 1), d.src_w);
  b.z1 = min(max(t[2] - d.D / 2, 0), max(b.depth - d.D, 0));
  b.y1 = min(max(t[3] - b.ch / 2, 0), d.src_h - b.ch);
  b.x1 = min(max(t[4] - b.cw / 2, 0), d.src_w - b.cw);
  return b;
}
// Rows resampled along z (the _z entries of lits3d.hip): the crop is cd slices deep, cd from zcrop[n] clamped
// into [1, zcrop_max]; the box is p3d_box's with cd in place of D.  cd is not clamped to the case: p3d_slice gives -1 beyond it.
__device__ __forceinline__ int p3d_zcrop(const int32_t* __restrict__ zcrop, int n, int zcrop_max) {
  return min(max(zcrop[n], 1), zcrop_max);
}
template <class Desc>
__device__ __forceinline__ Box3 p3d_box_z(const int32_t* __restrict__ t, const Desc& d, int cd) {
  Box3 b = p3d_box(t, d);
  b.z1 = (int)min(max((int64_t)t[2] - cd / 2, (int64_t)0), (int64_t)max(b.depth - cd, 0));
  return b;
}
// store index of crop slice z, or -1 where the crop leaves the case (or the store): zeros, label 0
template <class Desc>
__device__ __forceinline__ int64_t p3d_slice(const Box3& b, int z, const Desc& d) {
  const int zs = b.z1 + z;
  const int64_t s = b.base + zs;
  return (zs < b.depth && s >= 0 && s < d.n_slices) ? s : -1;
}

// ------------------------------------------------------------------------------------------------ block reductions
// Partials of one block, the same layout in every pass (workspace: sums[N][P][3] doubles, then minmax[N][P][2] floats):
//   sums   = {number of values, their sum, their sum of squares}
//   minmax = {min, max}                       (written by the patch pass only)
// Each is reduced in a fixed order: an xor butterfly inside the wave, then the four waves by index.
__device__ __forceinline__ void block_sum3(double cnt, double sum, double sq, double* __restrict__ dst) {
  __shared__ double sh[4][3];
  cnt = wave_sum_d(cnt);
  sum = wave_sum_d(sum);
  sq = wave_sum_d(sq);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sh[wave][0] = cnt;
    sh[wave][1] = sum;
    sh[wave][2] = sq;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double r0 = 0., r1 = 0., r2 = 0.;
    for (int w = 0; w < 4; ++w) {
      r0 += sh[w][0];
      r1 += sh[w][1];
      r2 += sh[w][2];
    }
    dst[0] = r0;
    dst[1] = r1;
    dst[2] = r2;
  }
  __syncthreads();
}
__device__ __forceinline__ void block_minmax(float lo, float hi, float* __restrict__ dst) {
  __shared__ float sh[4][2];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o));
    hi = fmaxf(hi, __shfl_xor(hi, o));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sh[wave][0] = lo;
    sh[wave][1] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      lo = fminf(lo, sh[w][0]);
      hi = fmaxf(hi, sh[w][1]);
    }
    dst[0] = lo;
    dst[1] = hi;
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------ finalising block
// One wave per sample walks the P partials by index (lane l takes l, l + 64, ...; then a fixed butterfly): mean and
// standard deviation of the values the pass counted, and in stage 1 their min and range.
//   stage 0 (mask moments)  -> m, s                    (empty mask: 0, 0)
//   stage 1 (patch)         -> mn, sd, min, range      of the normalised patch
//   stage 2 (gamma)         -> new_mn, new_sd          of the gamma-mapped patch
__global__ __launch_bounds__(64) void p3d_finalize_kernel(int stage, int P, const double* __restrict__ part,
                                                          const float* __restrict__ minmax, float* __restrict__ stat) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const double* p = part + (int64_t)n * P * 3;
  const float* mm = minmax + (int64_t)n * P * 2;
  double cnt = 0., sum = 0., sq = 0.;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = lane; i < P; i += 64) {
    cnt += p[i * 3 + 0];
    sum += p[i * 3 + 1];
    sq += p[i * 3 + 2];
    if (stage == 1) {
      lo = fminf(lo, mm[i * 2 + 0]);
      hi = fmaxf(hi, mm[i * 2 + 1]);
    }
  }
  cnt = wave_sum_d(cnt);
  sum = wave_sum_d(sum);
  sq = wave_sum_d(sq);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o));
    hi = fmaxf(hi, __shfl_xor(hi, o));
  }
  if (lane != 0) return;
  double m = 0., var = 0.;
  if (cnt > 0.) {
    m = sum / cnt;
    var = fmax(sq / cnt - m * m, 0.);
  }
  float* st = stat + (int64_t)n * ST_N;
  if (stage == 0) {
    st[ST_M] = (float)m;
    st[ST_S] = (float)sqrt(var);
  } else if (stage == 1) {
    st[ST_MN] = (float)m;
    st[ST_SD] = (float)sqrt(var);
    st[ST_MIN] = lo;
    st[ST_RNG] = hi - lo;
  } else {
    st[ST_NMN] = (float)m;
    st[ST_NSD] = (float)sqrt(var);
  }
}

// ------------------------------------------------------------------------------------------------ gamma
// augment_gamma (image_ops.py:339-354), retain_stats=True, in float32 as the reference: the accurate powf.  `total` = the
// values of one sample (< 2^31: checked by the entry points).
__global__ __launch_bounds__(256) void p3d_gamma_kernel(int total, const int32_t* __restrict__ tab,
                                                        const float* __restrict__ stat, float* __restrict__ images,
                                                        double* __restrict__ part) {
  const int n = blockIdx.y, P = gridDim.x;
  const float gamma = __int_as_float(tab[(int64_t)n * TW + 10]);
  const float* st = stat + (int64_t)n * ST_N;
  const float minm = st[ST_MIN], rnge = st[ST_RNG];
  float* img = images + (int64_t)n * total;
  double cnt = 0., sum = 0., sq = 0.;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += P * 256) {
    const float y = powf((img[i] - minm) / (rnge + 1e-7f), gamma) * rnge + minm;
    img[i] = y;
    cnt += 1.;
    sum += (double)y;
    sq += (double)y * (double)y;
  }
  block_sum3(cnt, sum, sq, part + ((int64_t)n * P + blockIdx.x) * 3);
}

__global__ __launch_bounds__(256) void p3d_retain_kernel(int total, const float* __restrict__ stat,
                                                         float* __restrict__ images) {
  const int n = blockIdx.y, P = gridDim.x;
  const float* st = stat + (int64_t)n * ST_N;
  const float mn = st[ST_MN], sd = st[ST_SD], nmn = st[ST_NMN], nden = st[ST_NSD] + 1e-8f;
  float* img = images + (int64_t)n * total;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += P * 256) img[i] = (img[i] - nmn + mn) / nden * sd;
}

}  // namespace
