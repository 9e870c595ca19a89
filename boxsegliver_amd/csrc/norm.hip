// Normalisation + activation passes around the conv kernels (HBM-bound, float4 NHWC).
//
// Replaces, after every slim.conv2d(x, C, 3) (NetworksV2/UNet.py:79,85,94; GUNet.py:181-188; UNet3D.py:153,165):
//   slim.batch_norm    (NetworksV2/base.py:153-162: eps 1e-3, decay .999 / .99 in GUNet's encoder, fused;
//                       training: batch mean + biased variance, unbiased variance into the moving average)
//   slim.instance_norm (base.py:163-165: eps 1e-6, moments over the spatial axes per (n, c))
//   optional centre / scale (GUNet.yml: norm_with_center true, norm_with_scale false, GUNet.py:313-330)
//   GUNet's density modulation  net * den[b, c]  (`conditional_normalization`, GUNet.py:119-133,203-206; den = a slice of
//     the context MLP's output) -- template flag D
//   GUNet's spatial modulation  net + sp_params[..., slice]  (GUNet.py:207-212) where sp_params is the
//     1x1 conv of the pooled guide (GUNet.py:154-156): computed on the fly, never materialised
//   ReLU
// i.e.  t = (y - mean) rstd gamma + beta,  u = t * den[b,c] + guide . gw + gb,  z = relu(u).
// gb without a guide (guide_ch == 0) is a bare per-channel shift after the gain: with den = gain * affine-gamma that is
// `after_affine` (slim_nets.channel_wise_affine, GUNet.py:213-214) folded into the same pass.
// The conv epilogue already produced per-tile sum / sum-of-squares partials, so the forward is one tiny
// finalise + ONE read-modify-write pass; the backward is two passes over (y, dz).
//
// One descriptor drives all of them.  STATISTICS groups: Ns = per_sample ? N : 1, each over P_stat pixels.  LAUNCH
// groups (blockIdx.y): L = N when the pass needs the sample index (instance norm, or density modulation under batch
// norm), else 1; a launch group indexes the statistics with stride sst (C or 0).
#include "common.h"

#include <algorithm>
#include <initializer_list>

namespace {

constexpr int MAXG = 4;   // guide channels

// adjacent row groups per pass in the plain norm kernels (measured: see norm_apply_relu_kernel); 1 = the plain loop
#ifndef UNETK_NORM_GROUPS
#define UNETK_NORM_GROUPS 4
#endif
// the same for bf16 storage (8-byte loads per thread: twice the groups keep the same bytes in flight) and for the reduction pass
#ifndef UNETK_NORM_GROUPS_BF
#define UNETK_NORM_GROUPS_BF 4
#endif
#ifndef UNETK_NORM_RGROUPS
#define UNETK_NORM_RGROUPS 2
#endif
#ifndef UNETK_NORM_RGROUPS_BF
#define UNETK_NORM_RGROUPS_BF 2
#endif

// Statistics geometry: any C > 0.  The finalise entry points and their query use nothing else.
struct StatGeom { int Ns; int64_t Ps; };   // statistic groups (1 for batch norm, N for instance norm), pixels per group
StatGeom stat_geom(const unetk_norm_desc* d) {
  return {d->per_sample ? d->N : 1, d->per_sample ? (int64_t)d->HW : (int64_t)d->N * d->HW};
}

// Launch geometry: only once C % 4 == 0 && C <= 1024 is established (unetk_colmap divides by C / 4, then 256 by the quotient).
struct LaunchGeom {
  int L;         // launch groups
  int64_t P;     // pixels per launch group
  int sst;       // statistics stride of a launch group (C or 0)
  int cq_n, rpi;
};
LaunchGeom launch_geom(const unetk_norm_desc* d, bool per_sample_groups) {
  const int L = (d->per_sample || per_sample_groups) ? d->N : 1;
  const ColMap m = unetk_colmap(d->C);
  return {L, L > 1 ? (int64_t)d->HW : (int64_t)d->N * d->HW, d->per_sample ? d->C : 0, m.cq_n, m.rows_per_iter};
}

// The batch statistics come in one pass, var = E[y^2] - E[y]^2 from fp32 partials: three fp32 roundings (the epilogue's row
// partials, the first-level row sums, the rounding of the sums below) each cost about 2^-24 (var + mean^2) of the
// variance, so its relative error grows with (mean / std)^2.  A channel is ill-conditioned when
// mean^2 > NORM_REFINE_T (var + eps); given the activations, its statistics are recomputed from them in a second, shifted
// pass (norm_refine_kernel).  T is derived in tests/test_norm_stats_host.py: the channels the one-pass path keeps stay
// well inside the 1e-5 relative rstd / variance bound of tests/test_gpu_norm_stats.py.  A flagged channel's recomputed
// statistics replace the one-pass ones only where these are off by more than that bound allows: 2^-16 (var + eps) of the
// variance (2^-17 of rstd), also 2^-17 of the variance where the moving variance is updated, 2^-23 |mean| + 2^-21 std of
// the mean.  A one-pass result within them stays, bit for bit.
constexpr double NORM_REFINE_T = 16.0;
constexpr int NORM_REFINE_PB = 64;         // at most this many pixel blocks per (group, 16 channels)
constexpr int64_t NORM_REFINE_PIX = 4096;  // pixels per pixel block, at least

int refine_blocks(int64_t Ps) {
  const int64_t b = (Ps + NORM_REFINE_PIX - 1) / NORM_REFINE_PIX;
  return (int)(b < 1 ? 1 : (b > NORM_REFINE_PB ? NORM_REFINE_PB : b));
}

// mean / var (float64) of one (group, channel) -> the moving statistics, mean / rstd / scale / shift
__device__ __forceinline__ void norm_finish(double m, double v, int c, int i, double count, const float* __restrict__ gamma,
                                            const float* __restrict__ beta, float eps, float decay, int update_moving,
                                            float* __restrict__ moving_mean, float* __restrict__ moving_var,
                                            float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                            float* __restrict__ scale_out, float* __restrict__ shift_out) {
  const float mean = (float)m, var = (float)v;
  if (update_moving) {   // batch norm only (Ns == 1)
    const double unbiased = count > 1.0 ? v * (count / (count - 1.0)) : v;
    moving_mean[c] = moving_mean[c] * decay + mean * (1.f - decay);
    moving_var[c] = moving_var[c] * decay + (float)unbiased * (1.f - decay);
  }
  const float rstd = 1.0f / sqrtf(var + eps);
  const float g = gamma ? gamma[c] : 1.f;
  const float b = beta ? beta[c] : 0.f;
  const float scale = g * rstd;
  mean_out[i] = mean;
  rstd_out[i] = rstd;
  scale_out[i] = scale;
  shift_out[i] = b - mean * scale;
}

// Last level of the statistics reduction fused with the finalisation: src[2][Ns][rows][C] (rows <= 256: the conv
// epilogue's partials, or their first-level sums) -> mean / rstd / scale / shift.  Block = 16 channels x 16 row lanes of
// one group; fp64 row sums in a fixed order, rounded to fp32 exactly as unetk_rows_reduce + norm_finalize_kernel did.
// flags != null (the activations were given): flags[g][c] = the channel is ill-conditioned; such a channel keeps its
// float64 one-pass mean / variance in one[g][c][2] and leaves its moving statistics to norm_refine_kernel, and the
// (group, 16-channel block)'s arrival counter is zeroed for it.
__global__ __launch_bounds__(256) void norm_reduce_finalize_kernel(
    const float* __restrict__ src, int rows, int Ns, int C, double count, const float* __restrict__ gamma,
    const float* __restrict__ beta, float eps, float decay, int update_moving, float* __restrict__ moving_mean,
    float* __restrict__ moving_var, float* __restrict__ mean_out, float* __restrict__ rstd_out,
    float* __restrict__ scale_out, float* __restrict__ shift_out, int* __restrict__ flags, unsigned* __restrict__ counters,
    double* __restrict__ one) {
  __shared__ double red[2][16][17];
  const int cblocks = (C + 15) / 16;
  const int cb = blockIdx.x % cblocks, gi = blockIdx.x / cblocks;
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int c = cb * 16 + cl;
  double s0 = 0.0, s1 = 0.0;
  if (c < C)
    for (int r = rl; r < rows; r += 16) {
      s0 += (double)src[((int64_t)gi * rows + r) * C + c];
      s1 += (double)src[((int64_t)(Ns + gi) * rows + r) * C + c];
    }
  red[0][rl][cl] = s0;
  red[1][rl][cl] = s1;
  __syncthreads();
  if (rl != 0 || c >= C) return;
  double t0 = 0.0, t1 = 0.0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    t0 += red[0][j][cl];
    t1 += red[1][j][cl];
  }
  const double m = (double)(float)t0 / count;
  double v = (double)(float)t1 / count - m * m;
  if (v < 0.0) v = 0.0;
  const int i = gi * C + c;
  int refine = 0;
  if (flags) {
    refine = m * m > NORM_REFINE_T * (v + (double)eps) ? 1 : 0;
    flags[i] = refine;
    if (refine) {
      one[2 * i] = m;
      one[2 * i + 1] = v;
    }
    if (cl == 0) counters[gi * cblocks + cb] = 0u;
  }
  norm_finish(m, v, c, i, count, gamma, beta, eps, decay, update_moving && !refine, moving_mean, moving_var, mean_out,
              rstd_out, scale_out, shift_out);
}

// The second pass of the flagged channels.  Grid = (group, 16-channel block, pixel block PB): a block whose 16 channels are
// all unflagged returns at once.  Block = four float4 channel lanes x 64 pixel lanes over one contiguous pixel range of
// the group; fp64 sums of d = y - p and d^2 with p = the one-pass fp32 mean (mean_out), in a fixed order (pixel lane ->
// groups of four lanes -> sixteen groups), into part[g][cb][PB][2][16].  The last block of a (group, channel block) to
// arrive sums the PB partials in block order,
//   mean = p + S1 / n,   var = S2 / n - (S1 / n)^2,
// and finishes the channel (mean / rstd / scale / shift, moving statistics) from these, or from the one-pass mean and
// variance in one[] where those are within the tolerances above.
// A constant channel has d = a few ulps of p at every pixel: every partial sum is exact and var is exactly 0.
__global__ __launch_bounds__(256) void norm_refine_kernel(
    const float* __restrict__ y, int64_t Ps, int Ns, int C, int PB, double count, const float* __restrict__ gamma,
    const float* __restrict__ beta, float eps, float decay, int update_moving, float* __restrict__ moving_mean,
    float* __restrict__ moving_var, float* __restrict__ mean_out, float* __restrict__ rstd_out,
    float* __restrict__ scale_out, float* __restrict__ shift_out, const int* __restrict__ flags,
    unsigned* __restrict__ counters, double* __restrict__ part, const double* __restrict__ one) {
  __shared__ double red[2][64][17];
  __shared__ double red2[2][16][17];
  __shared__ int last;
  const int cblocks = (C + 15) / 16;
  const int pb = blockIdx.x % PB;
  const int cb = (blockIdx.x / PB) % cblocks, gi = blockIdx.x / (PB * cblocks);
  const int fc = cb * 16 + (int)threadIdx.x;
  const int f = (threadIdx.x < 16 && fc < C) ? flags[gi * C + fc] : 0;
  if (!__syncthreads_or(f)) return;
  const int q = threadIdx.x & 3, rl = threadIdx.x >> 2;
  const int c0 = cb * 16 + q * 4;
  double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0};
  if (c0 < C) {   // C % 4 == 0
    const float4 p = ldg4(mean_out + (int64_t)gi * C + c0);
    const int64_t chunk = (Ps + PB - 1) / PB;
    const int64_t r0 = pb * chunk, r1 = r0 + chunk < Ps ? r0 + chunk : Ps;
    const float* yg = y + (int64_t)gi * Ps * C + c0;
    for (int64_t r = r0 + rl; r < r1; r += 64) {
      const float4 v = ldg4(yg + r * C);
      const double d0 = (double)v.x - (double)p.x, d1 = (double)v.y - (double)p.y;
      const double d2 = (double)v.z - (double)p.z, d3 = (double)v.w - (double)p.w;
      s0[0] += d0; s1[0] += d0 * d0;
      s0[1] += d1; s1[1] += d1 * d1;
      s0[2] += d2; s1[2] += d2 * d2;
      s0[3] += d3; s1[3] += d3 * d3;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    red[0][rl][q * 4 + k] = s0[k];
    red[1][rl][q * 4 + k] = s1[k];
  }
  __syncthreads();
  {
    const int cl = threadIdx.x & 15, j = threadIdx.x >> 4;
    red2[0][j][cl] = (red[0][4 * j][cl] + red[0][4 * j + 1][cl]) + (red[0][4 * j + 2][cl] + red[0][4 * j + 3][cl]);
    red2[1][j][cl] = (red[1][4 * j][cl] + red[1][4 * j + 1][cl]) + (red[1][4 * j + 2][cl] + red[1][4 * j + 3][cl]);
  }
  __syncthreads();
  double* pp = part + (((int64_t)gi * cblocks + cb) * PB + pb) * 32;
  if (threadIdx.x < 16) {
    double t0 = 0.0, t1 = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      t0 += red2[0][j][threadIdx.x];
      t1 += red2[1][j][threadIdx.x];
    }
    pp[threadIdx.x] = t0;
    pp[16 + threadIdx.x] = t1;
    __threadfence();
  }
  __syncthreads();
  if (threadIdx.x == 0) last = atomicAdd(counters + gi * cblocks + cb, 1u) == (unsigned)(PB - 1);
  __syncthreads();
  if (!last || threadIdx.x >= 16 || fc >= C || !f) return;
  __threadfence();
  const double* pc = part + ((int64_t)gi * cblocks + cb) * PB * 32 + threadIdx.x;
  double S0 = 0.0, S1 = 0.0;
  for (int b = 0; b < PB; ++b) {
    S0 += __hip_atomic_load(pc + b * 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    S1 += __hip_atomic_load(pc + b * 32 + 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const int i = gi * C + fc;
  const double dm = S0 / count;
  double v = S1 / count - dm * dm;
  if (v < 0.0) v = 0.0;
  const double m = (double)mean_out[i] + dm;
  const double m1 = one[2 * i], v1 = one[2 * i + 1];
  const double dv = fabs(v1 - v);
  const bool keep = dv <= 0x1p-16 * (v + (double)eps) && (!update_moving || dv <= 0x1p-17 * v) &&
                    fabs(m1 - m) <= 0x1p-23 * fabs(m) + 0x1p-21 * sqrt(v);
  norm_finish(keep ? m1 : m, keep ? v1 : v, fc, i, count, gamma, beta, eps, decay, update_moving, moving_mean, moving_var,
              mean_out, rstd_out, scale_out, shift_out);
}

// sums[0][g][c] = sum y, sums[1][g][c] = sum y^2 over `count` elements of group g
__global__ void norm_finalize_kernel(const float* __restrict__ sums, int Ns, int C, double count,
                                     const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                     float decay, int use_moving, int update_moving, float* __restrict__ moving_mean,
                                     float* __restrict__ moving_var, float* __restrict__ mean_out,
                                     float* __restrict__ rstd_out, float* __restrict__ scale_out,
                                     float* __restrict__ shift_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Ns * C) return;
  const int c = i % C;
  float mean, var;
  if (!use_moving) {
    const double m = (double)sums[i] / count;
    double v = (double)sums[Ns * C + i] / count - m * m;
    if (v < 0.0) v = 0.0;
    mean = (float)m;
    var = (float)v;
    if (update_moving) {   // batch norm only (Ns == 1)
      const double unbiased = count > 1.0 ? v * (count / (count - 1.0)) : v;
      moving_mean[c] = moving_mean[c] * decay + mean * (1.f - decay);
      moving_var[c] = moving_var[c] * decay + (float)unbiased * (1.f - decay);
    }
  } else {
    mean = moving_mean[c];
    var = moving_var[c];
  }
  const float rstd = 1.0f / sqrtf(var + eps);
  const float g = gamma ? gamma[c] : 1.f;
  const float b = beta ? beta[c] : 0.f;
  const float scale = g * rstd;
  mean_out[i] = mean;
  rstd_out[i] = rstd;
  scale_out[i] = scale;
  shift_out[i] = b - mean * scale;
}

struct ApplyArgs {
  const void* y;        // T = float, or bf16_t under d->storage == UNETK_BF16S (then z is bf16 too)
  const float* scale;   // [Ns][C]
  const float* shift;
  const float* den;     // [N][C] or null
  const float* guide;   // [N*HW][G] or null
  const float* gw;      // [G][gw_stride], columns gw_coff ..
  const float* gb;      // [gw_stride]
  void* z;
  int64_t P;
  int C, zs, cq_n, rpi, gw_stride, gw_coff, sst;
  int gw_ns, gb_ns;     // per-sample strides of gw / gb (0 = shared by the batch)
  int post;             // guide_leaky == 3: per-channel slopes + post-shift in the gb block (see post_act)
  float alpha;          // leaky slope of the guide branch (L)
  float keep;           // dropout keep probability, 0 = no dropout
  uint32_t seed;
};

__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// LGNet's guide branch (LGNet.py:30-55): the 1x1 guide conv has a leaky-ReLU activation (tf.nn.leaky_relu, alpha 0.2)
// before it is added: u = t + lrelu(guide . gw + gb) -- template flag L (without density modulation).
// alpha = d->guide_alpha: 0.2 for LGNet, 0 (plain ReLU) for GUNet --fix
__device__ __forceinline__ float lrelu(float s, float al) { return s > 0.f ? s : al * s; }
__device__ __forceinline__ float lrelu_grad(float s, float al) { return s > 0.f ? 1.f : al; }
// guide_leaky == 3 ("post"): the guide branch's activation has PER-CHANNEL slopes for s > 0 / s <= 0 and a per-channel shift is
// added behind it: u = t * den + (s > 0 ? ap : an) * s + ps, s = guide . gw + gb.  This is GUNet after_affine with --fix,
//   (t * den + relu(sg)) * gamma' + beta' = t * (den gamma') + gamma' relu(sg) + beta',
// with gamma' folded into gw / gb on the host (s = gamma' sg): gamma' relu(sg) = relu(s) where gamma' >= 0 (slopes 1, 0) and
// = min(s, 0) where gamma' < 0 (slopes 0, 1).  The gb block is then [4][gw_stride]: bias, ap, an, ps.
struct PostV { float4 ap, an, ps; };
__device__ __forceinline__ float4 post_act(const float4& s, const PostV& q) {
  return make_float4((s.x > 0.f ? q.ap.x : q.an.x) * s.x + q.ps.x, (s.y > 0.f ? q.ap.y : q.an.y) * s.y + q.ps.y,
                     (s.z > 0.f ? q.ap.z : q.an.z) * s.z + q.ps.z, (s.w > 0.f ? q.ap.w : q.an.w) * s.w + q.ps.w);
}
__device__ __forceinline__ float4 post_slope(const float4& s, const PostV& q) {
  return make_float4(s.x > 0.f ? q.ap.x : q.an.x, s.y > 0.f ? q.ap.y : q.an.y, s.z > 0.f ? q.ap.z : q.an.z, s.w > 0.f ? q.ap.w : q.an.w);
}
__device__ __forceinline__ PostV post_load(const float* gb_chan, int gw_stride) {
  PostV q;
  q.ap = ldg4(gb_chan + gw_stride); q.an = ldg4(gb_chan + 2 * gw_stride); q.ps = ldg4(gb_chan + 3 * gw_stride);
  return q;
}

// slim.dropout between the two convs of a modulated block (GUNet.py:189-190): the mask multiplies the NORMALISED value
// before the density gain / guide term; kept entries are scaled by 1 / keep.  Regenerated from (seed, element) in every pass.
__device__ __forceinline__ float4 drop4(uint32_t seed, uint32_t idx, float keep, float inv_keep) {
  return make_float4(unetk_uniform(seed, idx) < keep ? inv_keep : 0.f, unetk_uniform(seed, idx + 1) < keep ? inv_keep : 0.f,
                     unetk_uniform(seed, idx + 2) < keep ? inv_keep : 0.f, unetk_uniform(seed, idx + 3) < keep ? inv_keep : 0.f);
}

// z = relu((y*scale + shift) [* den] [+ guide . gw + gb])
template <int G, bool D, bool L = false, typename T = float>
__global__ __launch_bounds__(256) void norm_apply_relu_kernel(ApplyArgs a) {
  static_assert(!(L && G == 0), "the leaky guide needs a guide");
  const T* ay = static_cast<const T*>(a.y);
  T* az = static_cast<T*>(a.z);
  const int cq = threadIdx.x % a.cq_n, rl = threadIdx.x / a.cq_n;
  if (rl >= a.rpi) return;
  const int n = blockIdx.y;
  float4 sc = ldg4(a.scale + (int64_t)n * a.sst + cq * 4);
  float4 sh = ldg4(a.shift + (int64_t)n * a.sst + cq * 4);
  if (D) {
    const float4 dn = ldg4(a.den + (int64_t)n * a.C + cq * 4);
    sc = mul4(sc, dn);
    sh = mul4(sh, dn);
  }
  float4 gwv[G > 0 ? G : 1];
  float4 gbv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.gb) gbv = ldg4(a.gb + (int64_t)n * a.gb_ns + a.gw_coff + cq * 4);   // guide bias, or a bare post-shift when G == 0
  PostV pq{};
  if (L && a.post) pq = post_load(a.gb + (int64_t)n * a.gb_ns + a.gw_coff + cq * 4, a.gw_stride);
  const bool drop = a.keep > 0.f;
  const float inv_keep = drop ? 1.0f / a.keep : 1.f;
  if (!L && !drop) sh = add4(sh, gbv);                 // with dropout the post-shift is added after the mask
  if (G > 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) gwv[g] = ldg4(a.gw + (int64_t)n * a.gw_ns + (int64_t)g * a.gw_stride + a.gw_coff + cq * 4);
  }
  const int64_t base = (int64_t)n * a.P;
  const int64_t pstep = (int64_t)gridDim.x * a.rpi;
  int64_t pix = (int64_t)blockIdx.x * a.rpi + rl;
  if (G == 0 && !L && !drop && UNETK_NORM_GROUPS > 1) {
    // plain units (every unit of UNet / UNet3D): NP ADJACENT row groups per pass, all loads issued before any is used.
    // Measured on the headline step: NP = 2 -> 84.0 to 79.4 us per launch; pairing pix with pix + grid stride instead
    // (two far-apart streams per block) was 7 % SLOWER than no pairing.
    constexpr int NP = sizeof(T) == 2 ? UNETK_NORM_GROUPS_BF : UNETK_NORM_GROUPS;
    for (pix = (int64_t)blockIdx.x * NP * a.rpi + rl; pix < a.P; pix += NP * pstep) {
      float4 v[NP];
#pragma unroll
      for (int j = 0; j < NP; ++j)
        if (pix + j * a.rpi < a.P) v[j] = ld4(ay + (base + pix + j * a.rpi) * a.C + cq * 4);
#pragma unroll
      for (int j = 0; j < NP; ++j)
        if (pix + j * a.rpi < a.P) {
          float4 u;
          u.x = unetk_relu(fmaf(v[j].x, sc.x, sh.x)); u.y = unetk_relu(fmaf(v[j].y, sc.y, sh.y));
          u.z = unetk_relu(fmaf(v[j].z, sc.z, sh.z)); u.w = unetk_relu(fmaf(v[j].w, sc.w, sh.w));
          st4(az + (base + pix + j * a.rpi) * a.zs + cq * 4, u);
        }
    }
    return;
  }
  for (; pix < a.P; pix += pstep) {
    const float4 v = ld4(ay + (base + pix) * a.C + cq * 4);
    float4 u;
    u.x = fmaf(v.x, sc.x, sh.x); u.y = fmaf(v.y, sc.y, sh.y); u.z = fmaf(v.z, sc.z, sh.z); u.w = fmaf(v.w, sc.w, sh.w);
    if (drop) {
      const float4 m = drop4(a.seed, (uint32_t)((base + pix) * a.C + cq * 4), a.keep, inv_keep);
      u.x *= m.x; u.y *= m.y; u.z *= m.z; u.w *= m.w;
      if (!L) u = add4(u, gbv);
    }
    if (L) {
      float4 s = gbv;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float gg = a.guide[(base + pix) * G + g];
        s.x = fmaf(gg, gwv[g].x, s.x); s.y = fmaf(gg, gwv[g].y, s.y); s.z = fmaf(gg, gwv[g].z, s.z); s.w = fmaf(gg, gwv[g].w, s.w);
      }
      if (a.post) u = add4(u, post_act(s, pq));
      else { u.x += lrelu(s.x, a.alpha); u.y += lrelu(s.y, a.alpha); u.z += lrelu(s.z, a.alpha); u.w += lrelu(s.w, a.alpha); }
    } else {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float gg = a.guide[(base + pix) * G + g];
        u.x = fmaf(gg, gwv[g].x, u.x); u.y = fmaf(gg, gwv[g].y, u.y); u.z = fmaf(gg, gwv[g].z, u.z); u.w = fmaf(gg, gwv[g].w, u.w);
      }
    }
    u.x = unetk_relu(u.x); u.y = unetk_relu(u.y); u.z = unetk_relu(u.z); u.w = unetk_relu(u.w);
    st4(az + (base + pix) * a.zs + cq * 4, u);
  }
}

// z = relu(y * scale + shift) AND p = max_pool2d(z, 2, 2) in one pass (plain units whose activation feeds the pool:
// ops.Conv3x3NormReluPool): a thread owns a window, writes its four z and their maximum -- the pool's read of z disappears.
template <typename T>
__global__ __launch_bounds__(256) void norm_apply_relu_pool_kernel(ApplyArgs a, void* pooled, int H, int W, int L) {
  const T* ay = static_cast<const T*>(a.y);
  T* az = static_cast<T*>(a.z);
  T* ap = static_cast<T*>(pooled);
  const int cq = threadIdx.x % a.cq_n, rl = threadIdx.x / a.cq_n;
  if (rl >= a.rpi) return;
  const int n = blockIdx.y;
  const float4 sc = ldg4(a.scale + (int64_t)n * a.sst + cq * 4);
  const float4 sh = ldg4(a.shift + (int64_t)n * a.sst + cq * 4);
  const int Wo = W >> 1;
  const int64_t per_img = (int64_t)(H >> 1) * Wo;
  const int64_t Q = a.P >> 2;
  for (int64_t q = (int64_t)blockIdx.x * a.rpi + rl; q < Q; q += (int64_t)gridDim.x * a.rpi) {
    const int64_t img = L > 1 ? n : q / per_img;
    const int64_t r = L > 1 ? q : q - img * per_img;
    const int ho = (int)(r / Wo), wo = (int)(r - (int64_t)ho * Wo);
    const int64_t pix = (img * H + 2 * ho) * W + 2 * wo;
    const int64_t off[4] = {0, 1, W, (int64_t)W + 1};
    float4 v[4], u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = ld4(ay + (pix + off[i]) * a.C + cq * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u[i].x = unetk_relu(fmaf(v[i].x, sc.x, sh.x)); u[i].y = unetk_relu(fmaf(v[i].y, sc.y, sh.y));
      u[i].z = unetk_relu(fmaf(v[i].z, sc.z, sh.z)); u[i].w = unetk_relu(fmaf(v[i].w, sc.w, sh.w));
      st4(az + (pix + off[i]) * a.zs + cq * 4, u[i]);
    }
    float4 m;          // rounding to the storage type is monotonic: max of the stored values = stored max
    m.x = unetk_max4_nan(u[0].x, u[1].x, u[2].x, u[3].x); m.y = unetk_max4_nan(u[0].y, u[1].y, u[2].y, u[3].y);
    m.z = unetk_max4_nan(u[0].z, u[1].z, u[2].z, u[3].z); m.w = unetk_max4_nan(u[0].w, u[1].w, u[2].w, u[3].w);
    st4(ap + (img * per_img + r) * a.C + cq * 4, m);
  }
}

struct BwdArgs {
  const void* y;        // T = float or bf16_t (d->storage): y, dz and dy share it
  const void* dz;
  const float* scale;   // [Ns][C]
  const float* shift;
  const float* mean;
  const float* rstd;
  const float* den;     // [N][C] or null
  const float* guide;
  const float* gw;
  const float* gb;
  const float* ksum;    // apply pass: k = 0 row at ksum + n*kst, k = 1 row at ksum + krow + n*kst
  float* partial;       // [K][L][nblk][C] (reduce pass)
  void* dy;
  int64_t P;
  float inv_ps;         // 1 / pixels per STATISTICS group
  int C, dzs, cq_n, rpi, gw_stride, gw_coff, L, plain, sst, kst, krow;
  int gw_ns, gb_ns;     // per-sample strides of gw / gb (0 = shared)
  float alpha, keep;
  uint32_t seed;
  int post;             // guide_leaky == 3 (see post_act)
};

// pass 1.  With dt = du * den (dt = du without density), du = dz * (u > 0), xhat = (y - mean) rstd, t = y*scale + shift:
//   partial[0] = sum dt, partial[1] = sum dt*xhat, partial[2+g] = sum du*guide_g,
//   D only: partial[2+G] = sum du (guide bias gradient), partial[3+G] = sum du*t (density gradient, per sample)
//   L: partial[2+g] = sum du*lrelu'(s)*guide_g, partial[2+G] = sum du*lrelu'(s)  (s = guide . gw + gb; with D as well the
//   guide-bias row 2+G holds this sum instead of sum du, and 3+G the density gradient: GUNet --fix with --use_context)
//   P (guide_leaky == 3, with D and L): one more row, partial[4+G] = sum du -- the gradient of the post-shift
template <int G, bool D, bool L = false, typename T = float, bool P = false>
__global__ __launch_bounds__(256) void norm_bwd_reduce_kernel(BwdArgs a) {
  static_assert(!P || (D && L), "the post vectors come with the leaky guide and the density gains");
  constexpr int K = 2 + G + (D ? 2 : (L ? 1 : 0)) + (P ? 1 : 0);
  const T* ay = static_cast<const T*>(a.y);
  const T* adz = static_cast<const T*>(a.dz);
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [K][rpi][C]
  const int cq = threadIdx.x % a.cq_n, rl = threadIdx.x / a.cq_n;
  const int n = blockIdx.y;
  float4 s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (rl < a.rpi) {
    const int64_t so = (int64_t)n * a.sst + cq * 4;
    const float4 mu = ldg4(a.mean + so), rs = ldg4(a.rstd + so), sc0 = ldg4(a.scale + so), sh0 = ldg4(a.shift + so);
    float4 dn = make_float4(1.f, 1.f, 1.f, 1.f);
    if (D) dn = ldg4(a.den + (int64_t)n * a.C + cq * 4);
    const float4 sc = D ? mul4(sc0, dn) : sc0;
    float4 sh = D ? mul4(sh0, dn) : sh0;
    float4 gwv[G > 0 ? G : 1];
    float4 gbv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.gb) gbv = ldg4(a.gb + (int64_t)n * a.gb_ns + a.gw_coff + cq * 4);
    PostV pq{};
    if (P) pq = post_load(a.gb + (int64_t)n * a.gb_ns + a.gw_coff + cq * 4, a.gw_stride);
    const bool drop = a.keep > 0.f;
    const float inv_keep = drop ? 1.0f / a.keep : 1.f;
    if (!L && !drop) sh = add4(sh, gbv);
    if (G > 0) {
#pragma unroll
      for (int g = 0; g < G; ++g) gwv[g] = ldg4(a.gw + (int64_t)n * a.gw_ns + (int64_t)g * a.gw_stride + a.gw_coff + cq * 4);
    }
    const int64_t base = (int64_t)n * a.P;
    const int64_t pstep = (int64_t)gridDim.x * a.rpi;
    int64_t pix = (int64_t)blockIdx.x * a.rpi + rl;
    if (G == 0 && !D && !L && !drop && UNETK_NORM_GROUPS > 1) {
      // plain units: two adjacent row groups per pass (four loads in flight), summed in pixel order (four groups measured
      // slower here -- 101 vs 105 us -- while they help the apply passes)
      constexpr int NP = sizeof(T) == 2 ? UNETK_NORM_RGROUPS_BF : UNETK_NORM_RGROUPS;
      for (pix = (int64_t)blockIdx.x * NP * a.rpi + rl; pix < a.P; pix += NP * pstep) {
        float4 v[NP], d[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          v[j] = d[j] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (pix + j * a.rpi < a.P) {
            v[j] = ld4(ay + (base + pix + j * a.rpi) * a.C + cq * 4);
            d[j] = ld4(adz + (base + pix + j * a.rpi) * a.dzs + cq * 4);
          }
        }
#pragma unroll
        for (int j = 0; j < NP; ++j) {
#define NBR2(f)                                                              \
  {                                                                          \
    const float du = fmaf(v[j].f, sc.f, sh.f) > 0.f ? d[j].f : 0.f;          \
    s[0].f += du;                                                            \
    s[1].f += du * ((v[j].f - mu.f) * rs.f);                                 \
  }
          NBR2(x) NBR2(y) NBR2(z) NBR2(w)
#undef NBR2
        }
      }
      pix = a.P;     // done: skip the single-group loop
    }
    for (; pix < a.P; pix += pstep) {
      const float4 v = ld4(ay + (base + pix) * a.C + cq * 4);
      const float4 d = ld4(adz + (base + pix) * a.dzs + cq * 4);
      float4 u;
      u.x = fmaf(v.x, sc.x, sh.x); u.y = fmaf(v.y, sc.y, sh.y); u.z = fmaf(v.z, sc.z, sh.z); u.w = fmaf(v.w, sc.w, sh.w);
      float4 m = make_float4(1.f, 1.f, 1.f, 1.f);    // dropout mask (0 or 1 / keep) on the normalised value
      if (drop) {
        m = drop4(a.seed, (uint32_t)((base + pix) * a.C + cq * 4), a.keep, inv_keep);
        u.x *= m.x; u.y *= m.y; u.z *= m.z; u.w *= m.w;
        if (!L) u = add4(u, gbv);
      }
      float gg[G > 0 ? G : 1];
      float4 ls = make_float4(1.f, 1.f, 1.f, 1.f);   // lrelu'(s) of the leaky guide branch
      if (L) {
        float4 sg = gbv;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          gg[g] = a.guide[(base + pix) * G + g];
          sg.x = fmaf(gg[g], gwv[g].x, sg.x); sg.y = fmaf(gg[g], gwv[g].y, sg.y); sg.z = fmaf(gg[g], gwv[g].z, sg.z); sg.w = fmaf(gg[g], gwv[g].w, sg.w);
        }
        if (P) {
          u = add4(u, post_act(sg, pq));
          ls = post_slope(sg, pq);
        } else {
          u.x += lrelu(sg.x, a.alpha); u.y += lrelu(sg.y, a.alpha); u.z += lrelu(sg.z, a.alpha); u.w += lrelu(sg.w, a.alpha);
          ls = make_float4(lrelu_grad(sg.x, a.alpha), lrelu_grad(sg.y, a.alpha), lrelu_grad(sg.z, a.alpha), lrelu_grad(sg.w, a.alpha));
        }
      } else {
#pragma unroll
        for (int g = 0; g < G; ++g) {
          gg[g] = a.guide[(base + pix) * G + g];
          u.x = fmaf(gg[g], gwv[g].x, u.x); u.y = fmaf(gg[g], gwv[g].y, u.y); u.z = fmaf(gg[g], gwv[g].z, u.z); u.w = fmaf(gg[g], gwv[g].w, u.w);
        }
      }
#define NBR(f)                                                                \
  {                                                                           \
    const float du = u.f > 0.f ? d.f : 0.f;                                   \
    const float dt = (D ? du * dn.f : du) * m.f;                              \
    const float dg = L ? du * ls.f : du;                                      \
    s[0].f += dt;                                                             \
    s[1].f += dt * ((v.f - mu.f) * rs.f);                                     \
    _Pragma("unroll") for (int g = 0; g < G; ++g) s[2 + g].f += dg * gg[g];  \
    if (D) {                                                                  \
      s[2 + G].f += dg;                                                       \
      s[3 + G].f += du * m.f * fmaf(v.f, sc0.f, sh0.f);                       \
      if (P) s[4 + G].f += du;                                                \
    } else if (L) {                                                           \
      s[2 + G].f += dg;                                                       \
    }                                                                         \
  }
      NBR(x) NBR(y) NBR(z) NBR(w)
#undef NBR
    }
#pragma unroll
    for (int k = 0; k < K; ++k) stg4(&smem[(k * a.rpi + rl) * a.C + cq * 4], s[k]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K * a.C; i += 256) {
    const int k = i / a.C, c = i - k * a.C;
    float t = 0.f;
    for (int j = 0; j < a.rpi; ++j) t += smem[(k * a.rpi + j) * a.C + c];
    a.partial[(((int64_t)k * a.L + n) * gridDim.x + blockIdx.x) * a.C + c] = t;
  }
}

// pass 2: dy = scale * (dt - sum_dt/Ps - xhat * sum_dt_xhat/Ps)   (sums over the STATISTICS group)
template <int G, bool D, bool L = false, typename T = float>
__global__ __launch_bounds__(256) void norm_bwd_apply_kernel(BwdArgs a) {
  const int cq = threadIdx.x % a.cq_n, rl = threadIdx.x / a.cq_n;
  if (rl >= a.rpi) return;
  const T* ay = static_cast<const T*>(a.y);
  const T* adz = static_cast<const T*>(a.dz);
  T* ady = static_cast<T*>(a.dy);
  const int n = blockIdx.y;
  const int64_t so = (int64_t)n * a.sst + cq * 4;
  const float4 mu = ldg4(a.mean + so), rs = ldg4(a.rstd + so), sc0 = ldg4(a.scale + so), sh0 = ldg4(a.shift + so);
  float4 dn = make_float4(1.f, 1.f, 1.f, 1.f);
  if (D) dn = ldg4(a.den + (int64_t)n * a.C + cq * 4);
  const float4 sc = D ? mul4(sc0, dn) : sc0;
  float4 sh = D ? mul4(sh0, dn) : sh0;
  float4 gwv[G > 0 ? G : 1];
  float4 gbv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.gb) gbv = ldg4(a.gb + (int64_t)n * a.gb_ns + a.gw_coff + cq * 4);   // guide bias, or a bare post-shift when G == 0
  PostV pq{};
  if (L && a.post) pq = post_load(a.gb + (int64_t)n * a.gb_ns + a.gw_coff + cq * 4, a.gw_stride);
  const bool drop = a.keep > 0.f;
  const float inv_keep = drop ? 1.0f / a.keep : 1.f;
  if (!L && !drop) sh = add4(sh, gbv);
  if (G > 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) gwv[g] = ldg4(a.gw + (int64_t)n * a.gw_ns + (int64_t)g * a.gw_stride + a.gw_coff + cq * 4);
  }
  float4 k1 = ldg4(a.ksum + (int64_t)n * a.kst + cq * 4), k2 = ldg4(a.ksum + a.krow + (int64_t)n * a.kst + cq * 4);
  k1.x *= a.inv_ps; k1.y *= a.inv_ps; k1.z *= a.inv_ps; k1.w *= a.inv_ps;
  k2.x *= a.inv_ps; k2.y *= a.inv_ps; k2.z *= a.inv_ps; k2.w *= a.inv_ps;
  if (a.plain) {   // no normalisation (--without_norm): dy = dt * scale
    k1 = make_float4(0.f, 0.f, 0.f, 0.f);
    k2 = k1;
  }
  const int64_t base = (int64_t)n * a.P;
  const int64_t pstep = (int64_t)gridDim.x * a.rpi;
  int64_t pix = (int64_t)blockIdx.x * a.rpi + rl;
  if (G == 0 && !D && !L && !drop && UNETK_NORM_GROUPS > 1) {
    // plain units: NP adjacent row groups per pass, 2 NP loads in flight (see norm_apply_relu_kernel): 130.1 -> 116.8 us
    constexpr int NP = sizeof(T) == 2 ? UNETK_NORM_GROUPS_BF : UNETK_NORM_GROUPS;
    for (pix = (int64_t)blockIdx.x * NP * a.rpi + rl; pix < a.P; pix += NP * pstep) {
      float4 v[NP], d[NP];
#pragma unroll
      for (int j = 0; j < NP; ++j)
        if (pix + j * a.rpi < a.P) {
          v[j] = ld4(ay + (base + pix + j * a.rpi) * a.C + cq * 4);
          d[j] = ld4(adz + (base + pix + j * a.rpi) * a.dzs + cq * 4);
        }
#pragma unroll
      for (int j = 0; j < NP; ++j)
        if (pix + j * a.rpi < a.P) {
          float4 o;
#define NBA2(f)                                                                     \
  {                                                                                 \
    const float du = fmaf(v[j].f, sc.f, sh.f) > 0.f ? d[j].f : 0.f;                 \
    o.f = sc0.f * (du - k1.f - ((v[j].f - mu.f) * rs.f) * k2.f);                    \
  }
          NBA2(x) NBA2(y) NBA2(z) NBA2(w)
#undef NBA2
          st4(ady + (base + pix + j * a.rpi) * a.C + cq * 4, o);
        }
    }
    return;
  }
  for (; pix < a.P; pix += pstep) {
    const float4 v = ld4(ay + (base + pix) * a.C + cq * 4);
    const float4 d = ld4(adz + (base + pix) * a.dzs + cq * 4);
    float4 u, o;
    u.x = fmaf(v.x, sc.x, sh.x); u.y = fmaf(v.y, sc.y, sh.y); u.z = fmaf(v.z, sc.z, sh.z); u.w = fmaf(v.w, sc.w, sh.w);
    float4 m = make_float4(1.f, 1.f, 1.f, 1.f);
    if (drop) {
      m = drop4(a.seed, (uint32_t)((base + pix) * a.C + cq * 4), a.keep, inv_keep);
      u.x *= m.x; u.y *= m.y; u.z *= m.z; u.w *= m.w;
      if (!L) u = add4(u, gbv);
    }
    if (L) {
      float4 sg = gbv;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float gg = a.guide[(base + pix) * G + g];
        sg.x = fmaf(gg, gwv[g].x, sg.x); sg.y = fmaf(gg, gwv[g].y, sg.y); sg.z = fmaf(gg, gwv[g].z, sg.z); sg.w = fmaf(gg, gwv[g].w, sg.w);
      }
      if (a.post) u = add4(u, post_act(sg, pq));
      else { u.x += lrelu(sg.x, a.alpha); u.y += lrelu(sg.y, a.alpha); u.z += lrelu(sg.z, a.alpha); u.w += lrelu(sg.w, a.alpha); }
    } else {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float gg = a.guide[(base + pix) * G + g];
        u.x = fmaf(gg, gwv[g].x, u.x); u.y = fmaf(gg, gwv[g].y, u.y); u.z = fmaf(gg, gwv[g].z, u.z); u.w = fmaf(gg, gwv[g].w, u.w);
      }
    }
#define NBA(f)                                          \
  {                                                     \
    const float du = u.f > 0.f ? d.f : 0.f;             \
    const float dt = (D ? du * dn.f : du) * m.f;        \
    const float xh = (v.f - mu.f) * rs.f;               \
    o.f = sc0.f * (dt - k1.f - xh * k2.f);              \
  }
    NBA(x) NBA(y) NBA(z) NBA(w)
#undef NBA
    st4(ady + (base + pix) * a.C + cq * 4, o);
  }
}

// parameter gradients from psum[k][c] = sum over launch groups of sums[k][l][c]
__global__ void norm_bwd_params_kernel(const float* __restrict__ psum, int C, int G, int density, float* __restrict__ dgamma,
                                       float* __restrict__ dbeta, float* __restrict__ dgw, float* __restrict__ dgb) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  if (dbeta) dbeta[c] = psum[c];
  if (dgamma) dgamma[c] = psum[C + c];
  if (dgb) dgb[c] = density ? psum[(int64_t)(2 + G) * C + c] : psum[c];   // density | leaky: the separate sum du [* lrelu']
  for (int g = 0; g < G; ++g) dgw[(int64_t)g * C + c] = psum[(int64_t)(2 + g) * C + c];
}

// per-sample guide weights (GUNet --fix under instance norm): dgw[n][g][c] / dgb[n][c] from sums[k][l = n][c]
__global__ void norm_bwd_guide_ps_kernel(const float* __restrict__ sums, int N, int C, int G, int kb, float* __restrict__ dgw,
                                         float* __restrict__ dgb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * C) return;
  const int n = i / C, c = i - n * C;
  if (dgb) dgb[i] = sums[((int64_t)kb * N + n) * C + c];
  for (int g = 0; g < G; ++g) dgw[((int64_t)n * G + g) * C + c] = sums[((int64_t)(2 + g) * N + n) * C + c];
}

// guide_leaky == 3: dgb block [groups][4][C] from src[k][groups][C] (the per-sample sums, or their total with groups = 1)
__global__ void norm_bwd_post_block_kernel(const float* __restrict__ src, int groups, int C, int G, float* __restrict__ dgb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= groups * C) return;
  const int n = i / C, c = i - n * C;
  float* o = dgb + (int64_t)n * 4 * C + c;
  o[0] = src[((int64_t)(2 + G) * groups + n) * C + c];
  o[C] = 0.f;
  o[2 * C] = 0.f;
  o[3 * C] = src[((int64_t)(4 + G) * groups + n) * C + c];
}

// GUNet --use_se: the SE gate reads pooled[b][c] = mean over the sample's pixels of the normalised conv output, so the
// loss reaches y a second time through it: dt gets the per-(sample, channel) constant g[b][c] / HW.  The norm backward is
// linear in dt, so that part is added in place afterwards:  dy += scale * (A[b][c] - xhat * k2[c]) with
// A = g / HW - mean over the statistics group, k2 = mean of (g / HW) * xhat over the group (both tiny, from the host).
template <typename T>
__global__ __launch_bounds__(256) void norm_se_bwd_add_kernel(const T* __restrict__ y, T* __restrict__ dy,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ scale, const float* __restrict__ A,
                                                              const float* __restrict__ k2, int64_t P, int C, int cq_n, int rpi,
                                                              int sst) {
  const int cq = threadIdx.x % cq_n, rl = threadIdx.x / cq_n;
  if (rl >= rpi) return;
  const int n = blockIdx.y;
  const int64_t so = (int64_t)n * sst + cq * 4;
  const float4 mu = ldg4(mean + so), rs = ldg4(rstd + so), sc = ldg4(scale + so);
  const float4 av = ldg4(A + (int64_t)n * C + cq * 4), kv = ldg4(k2 + so);
  const int64_t base = (int64_t)n * P;
  for (int64_t pix = (int64_t)blockIdx.x * rpi + rl; pix < P; pix += (int64_t)gridDim.x * rpi) {
    const float4 v = ld4(y + (base + pix) * C + cq * 4);
    float4 o = ld4(dy + (base + pix) * C + cq * 4);
    o.x += sc.x * (av.x - (v.x - mu.x) * rs.x * kv.x);
    o.y += sc.y * (av.y - (v.y - mu.y) * rs.y * kv.y);
    o.z += sc.z * (av.z - (v.z - mu.z) * rs.z * kv.z);
    o.w += sc.w * (av.w - (v.w - mu.w) * rs.w * kv.w);
    st4(dy + (base + pix) * C + cq * 4, o);
  }
}

// GUNet --use_se with --dropout (GUNet.py:189-201): the gate pools the DROPPED-OUT normalised output,
//   pooled[b][c] = mean_p m_p (gamma xhat_p + beta) = gamma * mean_p(m_p xhat_p) + beta * mean_p(m_p),
// which does not follow from the conv's statistic partials: sums[0][b][c] = sum_p m_p xhat_p, sums[1][b][c] = sum_p m_p, the mask
// regenerated from (seed, element index) as in the apply / backward passes.  One block per sample, fixed summation order.
template <typename T>
__global__ __launch_bounds__(256) void norm_drop_pool_kernel(const T* __restrict__ y, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, float* __restrict__ sums, int64_t P,
                                                             int C, int cq_n, int rpi, int sst, int N, float keep, uint32_t seed) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [2][rpi][C]
  const int cq = threadIdx.x % cq_n, rl = threadIdx.x / cq_n;
  const int n = blockIdx.x;
  float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
  if (rl < rpi) {
    const int64_t so = (int64_t)n * sst + cq * 4;
    const float4 mu = ldg4(mean + so), rs = ldg4(rstd + so);
    const float inv_keep = 1.0f / keep;
    const int64_t base = (int64_t)n * P;
    for (int64_t pix = rl; pix < P; pix += rpi) {
      const float4 v = ld4(y + (base + pix) * C + cq * 4);
      const float4 m = drop4(seed, (uint32_t)((base + pix) * C + cq * 4), keep, inv_keep);
      s0.x += m.x * ((v.x - mu.x) * rs.x); s0.y += m.y * ((v.y - mu.y) * rs.y);
      s0.z += m.z * ((v.z - mu.z) * rs.z); s0.w += m.w * ((v.w - mu.w) * rs.w);
      s1.x += m.x; s1.y += m.y; s1.z += m.z; s1.w += m.w;
    }
    stg4(&smem[(0 * rpi + rl) * C + cq * 4], s0);
    stg4(&smem[(1 * rpi + rl) * C + cq * 4], s1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += 256) {
    const int k = i / C, c = i - k * C;
    float t = 0.f;
    for (int j = 0; j < rpi; ++j) t += smem[(k * rpi + j) * C + c];
    sums[((int64_t)k * N + n) * C + c] = t;
  }
}

// ... and its way back: dt gets m_p * E[b][c] (E = d loss / d pooled / HW), and the norm backward being linear in dt,
//   dy += scale * (m_p E[b][c] - k1 - xhat k2),  k1 / k2 = the statistics group's means of m E and m E xhat (from the host:
// they follow from the two sums above).
template <typename T>
__global__ __launch_bounds__(256) void norm_se_bwd_add_drop_kernel(const T* __restrict__ y, T* __restrict__ dy,
                                                                   const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                   const float* __restrict__ scale, const float* __restrict__ E,
                                                                   const float* __restrict__ k1, const float* __restrict__ k2,
                                                                   int64_t P, int C, int cq_n, int rpi, int sst, float keep,
                                                                   uint32_t seed) {
  const int cq = threadIdx.x % cq_n, rl = threadIdx.x / cq_n;
  if (rl >= rpi) return;
  const int n = blockIdx.y;
  const int64_t so = (int64_t)n * sst + cq * 4;
  const float4 mu = ldg4(mean + so), rs = ldg4(rstd + so), sc = ldg4(scale + so);
  const float4 ev = ldg4(E + (int64_t)n * C + cq * 4), k1v = ldg4(k1 + so), k2v = ldg4(k2 + so);
  const float inv_keep = 1.0f / keep;
  const int64_t base = (int64_t)n * P;
  for (int64_t pix = (int64_t)blockIdx.x * rpi + rl; pix < P; pix += (int64_t)gridDim.x * rpi) {
    const float4 v = ld4(y + (base + pix) * C + cq * 4);
    const float4 m = drop4(seed, (uint32_t)((base + pix) * C + cq * 4), keep, inv_keep);
    float4 o = ld4(dy + (base + pix) * C + cq * 4);
    o.x += sc.x * (m.x * ev.x - k1v.x - (v.x - mu.x) * rs.x * k2v.x);
    o.y += sc.y * (m.y * ev.y - k1v.y - (v.y - mu.y) * rs.y * k2v.y);
    o.z += sc.z * (m.z * ev.z - k1v.z - (v.z - mu.z) * rs.z * k2v.z);
    o.w += sc.w * (m.w * ev.w - k1v.w - (v.w - mu.w) * rs.w * k2v.w);
    st4(dy + (base + pix) * C + cq * 4, o);
  }
}

bool norm_desc_ok(const unetk_norm_desc* d) {
  return d && d->N > 0 && d->HW > 0 && d->C > 0 && d->guide_ch >= 0 && d->guide_ch <= MAXG;
}
bool norm_supported(const unetk_norm_desc* d) { return d->C % 4 == 0 && d->C <= 1024; }

int bwd_blocks(const LaunchGeom& g) {
  const int64_t b = (g.P + g.rpi - 1) / g.rpi;
  // per launch group; few groups (instance norm at batch 1-2: UNet3D's 96^3 tensors) need more blocks each to fill the GPU
  const int64_t cap = g.L > 1 ? (2048 / g.L > 64 ? 2048 / g.L : 64) : UNETK_COL_BLOCKS;
  return (int)(b > cap ? cap : b);
}

// blocks of an apply pass, per launch group, over `pixels` rows of work (P, or the P / 4 windows of the pool pair)
int apply_grid(int64_t pixels, const LaunchGeom& g) {
  const int64_t b = (pixels + g.rpi - 1) / g.rpi;
  const int64_t cap = g.L > 1 ? (4096 + g.L - 1) / g.L : 4096;
  return (int)(b > cap ? cap : b);
}

// the tensors of a call are float (16-byte accesses) or bf16_t (8-byte); no other storage has kernels
bool norm_storage_ok(int storage, std::initializer_list<const void*> tensors) {
  bool ok = storage == UNETK_FP32 || storage == UNETK_BF16S;
  for (const void* p : tensors) ok = ok && (storage == UNETK_BF16S ? unetk_aligned8(p) : unetk_aligned16(p));
  return ok;
}

// a guide comes with its weights and its gb block (columns gw_coff .. gw_coff + C of rows gw_stride wide); gb alone is a bare shift
bool guide_operands_ok(const unetk_norm_desc* d, const float* guide, const float* gw, const float* gb) {
  if (d->guide_ch > 0 &&
      !(guide && gw && gb && d->gw_stride >= d->gw_coff + d->C && d->gw_stride % 4 == 0 && unetk_aligned16(gw)))
    return false;
  return !gb || (d->gw_coff % 4 == 0 && d->gw_coff >= 0 && unetk_aligned16(gb));
}

// the call is the variadic part: once expanded, its commas stand outside parentheses
#define GL_DISPATCH(G_, ...) \
  switch (G_) {              \
    case 1: { constexpr int GG = 1; __VA_ARGS__; } break; \
    case 2: { constexpr int GG = 2; __VA_ARGS__; } break; \
    case 3: { constexpr int GG = 3; __VA_ARGS__; } break; \
    default: { constexpr int GG = 4; __VA_ARGS__; } break; \
  }
#define G_DISPATCH(G_, ...)                              \
  if (G_ == 0) { constexpr int GG = 0; __VA_ARGS__; } \
  else GL_DISPATCH(G_, __VA_ARGS__)
#define GD_DISPATCH_T(TT, G_, D_, L_, KERN, ...)                                               \
  if (L_ && D_) { GL_DISPATCH(G_, UNETK_LAUNCH((KERN<GG, true, true, TT>), __VA_ARGS__)); } \
  else if (L_) { GL_DISPATCH(G_, UNETK_LAUNCH((KERN<GG, false, true, TT>), __VA_ARGS__)); }   \
  else if (D_) { G_DISPATCH(G_, UNETK_LAUNCH((KERN<GG, true, false, TT>), __VA_ARGS__)); } \
  else { G_DISPATCH(G_, UNETK_LAUNCH((KERN<GG, false, false, TT>), __VA_ARGS__)); }
// S_: tensors in HBM are bf16 (UNETK_BF16S) instead of fp32
#define GD_DISPATCH(S_, G_, D_, L_, KERN, ...)                      \
  if (S_) { GD_DISPATCH_T(bf16_t, G_, D_, L_, KERN, __VA_ARGS__) } \
  else { GD_DISPATCH_T(float, G_, D_, L_, KERN, __VA_ARGS__) }
// CALL for the storage type of the tensors, which it names TT (the kernels that GD_DISPATCH does not cover)
#define T_DISPATCH(S_, CALL)             \
  if (S_) { using TT = bf16_t; CALL; } \
  else { using TT = float; CALL; }

// ---- plain unit whose activation feeds a 2 x 2 max-pool AND the skip connection (UNet.py:80-81,93: every encoder level's
// second conv): the pool's backward is folded into both passes.  dz of pixel i of a window = dskip_i + (i is the window's
// first maximum of z ? dp : 0) (TF MaxPoolGrad's rule, pool.hip), with z = relu(y * scale + shift) re-evaluated from y by the
// forward's own expression and rounded as the forward stored it; the sum is rounded to the storage type as the separate
// pool-backward pass stored it.  Saves that pass: 3.25 tensor transits of the 8.25 the three passes moved.
struct PoolArgs {
  const void* dp;       // [N][H/2][W/2][C], dense
  int H, W;
};
template <typename T>
__device__ __forceinline__ float round_as(float v);
template <>
__device__ __forceinline__ float round_as<float>(float v) { return v; }
template <>
__device__ __forceinline__ float round_as<bf16_t>(float v) { return unetk_round_bf16(v); }

// window q of launch group n -> its four pixels' y, routed dz (d) and masked gradient du; f(pixel, y, du) per pixel
template <typename T, class F>
__device__ __forceinline__ void pool_window(const BwdArgs& a, const PoolArgs& pa, int n, int64_t q, int cq, const float4& sc,
                                            const float4& sh, F&& f) {
  const int Wo = pa.W >> 1;
  const int64_t per_img = (int64_t)(pa.H >> 1) * Wo;
  const int64_t img = a.L > 1 ? n : q / per_img;
  const int64_t r = a.L > 1 ? q : q - img * per_img;
  const int ho = (int)(r / Wo), wo = (int)(r - (int64_t)ho * Wo);
  const int64_t pix = (img * pa.H + 2 * ho) * pa.W + 2 * wo;               // global pixel index of the window's corner
  const int64_t off[4] = {0, 1, pa.W, (int64_t)pa.W + 1};
  const T* ay = static_cast<const T*>(a.y);
  const T* ask = static_cast<const T*>(a.dz);
  float4 v[4], d[4], u[4], z[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = ld4(ay + (pix + off[i]) * a.C + cq * 4);
    d[i] = ld4(ask + (pix + off[i]) * a.dzs + cq * 4);
  }
  const float4 g = ld4(static_cast<const T*>(pa.dp) + ((img * per_img + r) * a.C + cq * 4));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u[i].x = fmaf(v[i].x, sc.x, sh.x); u[i].y = fmaf(v[i].y, sc.y, sh.y); u[i].z = fmaf(v[i].z, sc.z, sh.z); u[i].w = fmaf(v[i].w, sc.w, sh.w);
    // backward only: fmaxf stays (unetk.h, non-finite contract) -- it decides which pixel of a finite window takes dp, where it
    // equals unetk_relu, and a NaN forward has refused the step before this runs
    z[i].x = round_as<T>(fmaxf(u[i].x, 0.f)); z[i].y = round_as<T>(fmaxf(u[i].y, 0.f));
    z[i].z = round_as<T>(fmaxf(u[i].z, 0.f)); z[i].w = round_as<T>(fmaxf(u[i].w, 0.f));
  }
#define PWIN(c)                                                                   \
  {                                                                               \
    const float m = fmaxf(fmaxf(z[0].c, z[1].c), fmaxf(z[2].c, z[3].c));          \
    const bool e0 = z[0].c == m;                                                  \
    const bool e1 = !e0 && z[1].c == m;                                           \
    const bool e2 = !e0 && !e1 && z[2].c == m;                                    \
    const bool e3 = !e0 && !e1 && !e2;                                            \
    d[0].c = round_as<T>(d[0].c + (e0 ? g.c : 0.f));                              \
    d[1].c = round_as<T>(d[1].c + (e1 ? g.c : 0.f));                              \
    d[2].c = round_as<T>(d[2].c + (e2 ? g.c : 0.f));                              \
    d[3].c = round_as<T>(d[3].c + (e3 ? g.c : 0.f));                              \
  }
  PWIN(x) PWIN(y) PWIN(z) PWIN(w)
#undef PWIN
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float4 du;
    du.x = u[i].x > 0.f ? d[i].x : 0.f; du.y = u[i].y > 0.f ? d[i].y : 0.f;
    du.z = u[i].z > 0.f ? d[i].z : 0.f; du.w = u[i].w > 0.f ? d[i].w : 0.f;
    f(pix + off[i], v[i], du);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void norm_bwd_reduce_pool_kernel(BwdArgs a, PoolArgs pa) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [2][rpi][C]
  const int cq = threadIdx.x % a.cq_n, rl = threadIdx.x / a.cq_n;
  const int n = blockIdx.y;
  float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
  if (rl < a.rpi) {
    const int64_t so = (int64_t)n * a.sst + cq * 4;
    const float4 mu = ldg4(a.mean + so), rs = ldg4(a.rstd + so), sc = ldg4(a.scale + so), sh = ldg4(a.shift + so);
    const int64_t Q = a.P >> 2;                                    // windows of this launch group
    for (int64_t q = (int64_t)blockIdx.x * a.rpi + rl; q < Q; q += (int64_t)gridDim.x * a.rpi)
      pool_window<T>(a, pa, n, q, cq, sc, sh, [&](int64_t, const float4& v, const float4& du) {
        s0.x += du.x; s0.y += du.y; s0.z += du.z; s0.w += du.w;
        s1.x += du.x * ((v.x - mu.x) * rs.x); s1.y += du.y * ((v.y - mu.y) * rs.y);
        s1.z += du.z * ((v.z - mu.z) * rs.z); s1.w += du.w * ((v.w - mu.w) * rs.w);
      });
    stg4(&smem[(0 * a.rpi + rl) * a.C + cq * 4], s0);
    stg4(&smem[(1 * a.rpi + rl) * a.C + cq * 4], s1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * a.C; i += 256) {
    const int k = i / a.C, c = i - k * a.C;
    float t = 0.f;
    for (int j = 0; j < a.rpi; ++j) t += smem[(k * a.rpi + j) * a.C + c];
    a.partial[(((int64_t)k * a.L + n) * gridDim.x + blockIdx.x) * a.C + c] = t;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void norm_bwd_apply_pool_kernel(BwdArgs a, PoolArgs pa) {
  const int cq = threadIdx.x % a.cq_n, rl = threadIdx.x / a.cq_n;
  if (rl >= a.rpi) return;
  T* ady = static_cast<T*>(a.dy);
  const int n = blockIdx.y;
  const int64_t so = (int64_t)n * a.sst + cq * 4;
  const float4 mu = ldg4(a.mean + so), rs = ldg4(a.rstd + so), sc = ldg4(a.scale + so), sh = ldg4(a.shift + so);
  float4 k1 = ldg4(a.ksum + (int64_t)n * a.kst + cq * 4), k2 = ldg4(a.ksum + a.krow + (int64_t)n * a.kst + cq * 4);
  k1.x *= a.inv_ps; k1.y *= a.inv_ps; k1.z *= a.inv_ps; k1.w *= a.inv_ps;
  k2.x *= a.inv_ps; k2.y *= a.inv_ps; k2.z *= a.inv_ps; k2.w *= a.inv_ps;
  if (a.plain) {
    k1 = make_float4(0.f, 0.f, 0.f, 0.f);
    k2 = k1;
  }
  const int64_t Q = a.P >> 2;
  for (int64_t q = (int64_t)blockIdx.x * a.rpi + rl; q < Q; q += (int64_t)gridDim.x * a.rpi)
    pool_window<T>(a, pa, n, q, cq, sc, sh, [&](int64_t pix, const float4& v, const float4& du) {
      float4 o;
      o.x = sc.x * (du.x - k1.x - ((v.x - mu.x) * rs.x) * k2.x);
      o.y = sc.y * (du.y - k1.y - ((v.y - mu.y) * rs.y) * k2.y);
      o.z = sc.z * (du.z - k1.z - ((v.z - mu.z) * rs.z) * k2.z);
      o.w = sc.w * (du.w - k1.w - ((v.w - mu.w) * rs.w) * k2.w);
      st4(ady + pix * a.C + cq * 4, o);
    });
}

// ---- one decision per apply / backward / side-pass call, as ConvPlan / WgPlan / DeconvPlan / Conv3dPlan.  norm_plan (pure host
// arithmetic, no HIP calls) derives from the descriptor, the kind of call and WHICH optional operands are present everything the
// entry points and unetk_norm_bwd_ws_bytes do: refusals, launch geometry, template variant, both grids, the route of the dy
// formula's sums, the tail launches, the workspace layout.  The entry points validate pointers, plan, launch; nothing below the
// plan refuses a shape, chooses a grid or computes an offset.  Return codes: the first rule a call breaks decides, in one order:
//   1. BADARG, entry point: the descriptor's ranges (norm_desc_ok), a missing required pointer, a stride below C
//   2. UNSUPPORTED, plan: C % 4, C > 1024, stride % 4; the pool pair's guide / leaky / dropout and W / HW rules; drop_pool's affine_only
//   3. BADARG, plan: the keep range (0, 1] of the two dropout side passes; the storage.  `shaped` from here on (the geometry is
//      defined); the pool pair and the side passes have no further plan rule
//   4. BADARG, entry point: alignment, the guide's operands and strides, den without dden, gb without dgb
//   5. WORKSPACE, entry point (backward): ws_bytes below the query -- which is 0 where 6a or 6c refuses: those keep their code
//   6. plan, `unit` calls: a. leaky without a guide (UNSUPPORTED)  b. post without density or gb, or with pre_partials (UNSUPPORTED)
//      c. dropout_keep outside [0, 1] (BADARG)  d. backward: dropout with a guide or gb but neither density nor leaky (UNSUPPORTED:
//      the guide-bias sum needs the density variant, pass den = 1)  e. guide_per_sample with one launch group (UNSUPPORTED)
//      f. pre_partials with guide, density, gb, dropout or affine_only (UNSUPPORTED)  g. pre_rows no multiple of L > 0 (BADARG)
enum NormCall { NORM_APPLY, NORM_BWD, NORM_POOL_APPLY, NORM_POOL_BWD, NORM_SE_ADD, NORM_SE_ADD_DROP, NORM_DROP_POOL };
struct NormOperands { bool den, gb, dgb, pre; int pre_rows; };   // which optional operands the call was given
enum { WS_PARTIAL, WS_SUMS, WS_PSUM, WS_TMP1, WS_TMP2, WS_END };
struct NormWs { size_t at[WS_END + 1]; };   // the backward's workspace in floats from its start; at[WS_END] = its size
struct NormPlan {
  int rc;
  bool shaped;                   // rules 2 and 3 passed
  StatGeom s;
  LaunchGeom g;
  int G, K;                      // guide channels; rows of the reduce pass
  bool D, leaky, post, gps, bs;  // density, leaky guide, guide_leaky == 3, per-sample guide weights, bf16 storage
  bool simple;                   // K = 2 and no dgb: d beta / d gamma ARE the two totals, written by the last reduction launch
  size_t lds;                    // [K][rpi][C] floats of the reduce pass (and of unetk_norm_drop_pool)
  int gw_ns, gb_ns;              // per-sample strides of gw / gb
  float alpha;
  int nblk, gx, pre_rows;        // per launch group: blocks of the reduce pass, of the apply pass; pre_partials rows
  int tot;                       // WS_ index of the sums over all launch groups: the per-group sums themselves when L == 1
  int ksum, kst, krow;           // the dy formula's sums: WS_ index, stride per launch group, offset of the second row
  int kb, groups;                // gps: the guide-bias row of the per-group sums; post: groups of the dgb block
  size_t dden;                   // D: float offset of the density-gradient rows [N][C]
  NormWs ws;
};

NormWs bwd_ws_layout(int K, int L, int nblk, int C) {
  NormWs w;
  w.at[WS_PARTIAL] = 0;                                                   // [K][L][nblk][C]
  w.at[WS_SUMS] = (size_t)K * L * nblk * C;                               // [K][L][C]: sums per launch group
  w.at[WS_PSUM] = w.at[WS_SUMS] + (size_t)K * L * C;                      // [K][C]: sums over groups
  w.at[WS_TMP1] = w.at[WS_PSUM] + (size_t)K * C;                          // pre-computed partials may have any row count
  w.at[WS_TMP2] = w.at[WS_TMP1] + unetk_rows_reduce_tmp_floats(K * L, UNETK_RR_DIRECT_ROWS + 1, C);
  w.at[WS_END] = w.at[WS_TMP2] + unetk_rows_reduce_tmp_floats(K, L, C);
  return w;
}

NormPlan norm_plan(const unetk_norm_desc* d, NormCall call, int stride, int W, NormOperands p) {
  NormPlan pl{};
  const bool pool = call == NORM_POOL_APPLY || call == NORM_POOL_BWD;
  const bool unit = call == NORM_APPLY || call == NORM_BWD;
  pl.rc = UNETK_E_UNSUPPORTED;
  if (!norm_supported(d) || stride % 4 != 0) return pl;
  if (pool && (d->guide_ch > 0 || d->guide_leaky || d->dropout_keep > 0.f)) return pl;
  if (pool && (W < 2 || (W & 1) || d->HW % W != 0 || ((d->HW / W) & 1))) return pl;
  if (call == NORM_DROP_POOL && d->affine_only) return pl;
  pl.rc = UNETK_E_BADARG;
  if ((call == NORM_SE_ADD_DROP || call == NORM_DROP_POOL) && !(d->dropout_keep > 0.f && d->dropout_keep <= 1.f)) return pl;
  if (!norm_storage_ok(d->storage, {})) return pl;
  pl.shaped = true;
  pl.s = stat_geom(d);
  pl.g = launch_geom(d, p.den || !(unit || pool));       // a side pass: one launch group per sample
  pl.G = d->guide_ch; pl.D = p.den; pl.leaky = d->guide_leaky != 0; pl.gps = d->guide_per_sample != 0;
  pl.post = d->guide_leaky == 3;                         // gb and dgb are then blocks: [4][C] ([N][4][C] per sample)
  pl.bs = d->storage == UNETK_BF16S;
  if (unit) {
    const bool drop = d->dropout_keep > 0.f;
    pl.rc = UNETK_E_UNSUPPORTED;
    if (pl.leaky && pl.G < 1) return pl;
    if (pl.post && (!p.den || !p.gb || p.pre)) return pl;
    if (d->dropout_keep < 0.f || d->dropout_keep > 1.f) { pl.rc = UNETK_E_BADARG; return pl; }
    if (call == NORM_BWD && drop && (p.gb || pl.G > 0) && !pl.D && !pl.leaky) return pl;
    if (pl.gps && pl.g.L != d->N) return pl;
    if (p.pre && (pl.G > 0 || pl.D || pl.leaky || p.gb || drop || d->affine_only)) return pl;
    if (p.pre && !(p.pre_rows > 0 && p.pre_rows % pl.g.L == 0)) { pl.rc = UNETK_E_BADARG; return pl; }
  }
  pl.rc = UNETK_OK;
  pl.K = unit ? 2 + pl.G + (pl.D ? 2 : (pl.leaky ? 1 : 0)) + (pl.post ? 1 : 0) : 2;
  pl.simple = pl.G == 0 && !pl.D && !pl.leaky && !p.dgb;
  pl.lds = (size_t)pl.K * pl.g.rpi * d->C * sizeof(float);
  pl.gw_ns = pl.gps ? pl.G * d->gw_stride : 0; pl.gb_ns = pl.gps ? (pl.post ? 4 : 1) * d->gw_stride : 0;
  pl.alpha = d->guide_leaky == 2 ? d->guide_alpha : 0.2f;
  pl.nblk = bwd_blocks(pl.g);
  pl.gx = apply_grid(pool ? pl.g.P >> 2 : pl.g.P, pl.g);
  pl.pre_rows = p.pre ? p.pre_rows / pl.g.L : 0;
  // the statistics sums of the dy formula: per launch group when the statistics are per sample, else the batch totals
  pl.tot = pl.g.L == 1 ? WS_SUMS : WS_PSUM;
  pl.ksum = d->per_sample ? WS_SUMS : pl.tot; pl.kst = d->per_sample ? d->C : 0; pl.krow = d->per_sample ? pl.g.L * d->C : d->C;
  pl.kb = (pl.D || pl.leaky) ? 2 + pl.G : 0; pl.groups = pl.gps ? d->N : 1;
  pl.ws = bwd_ws_layout(pl.K, pl.g.L, pl.nblk, d->C);
  pl.dden = pl.ws.at[WS_SUMS] + (size_t)(3 + pl.G) * pl.g.L * d->C;     // the per-sample row sum du * t
  return pl;
}

// what the plain and the pool-fused apply pass share (the pool kernel reads neither density, guide nor dropout fields)
ApplyArgs apply_args(const unetk_norm_desc* d, const NormPlan& pl, const void* y, const float* scale, const float* shift,
                     const float* den, const float* guide, const float* gw, const float* gb, void* z) {
  return ApplyArgs{y, scale, shift, den, guide, gw, gb, z, pl.g.P, d->C, d->z_stride, pl.g.cq_n, pl.g.rpi, d->gw_stride,
                   d->gw_coff, pl.g.sst, pl.gw_ns, pl.gb_ns, pl.post ? 1 : 0, pl.alpha, d->dropout_keep, d->dropout_seed};
}

// both passes of a backward, plain or pool-fused (dz = dskip there)
BwdArgs bwd_args(const unetk_norm_desc* d, const NormPlan& pl, float* ws, const void* y, const void* dz, int dz_stride,
                 const float* scale, const float* shift, const float* mean, const float* rstd, const float* den,
                 const float* guide, const float* gw, const float* gb, void* dy) {
  BwdArgs a{};
  a.y = y; a.dz = dz; a.scale = scale; a.shift = shift; a.mean = mean; a.rstd = rstd; a.den = den;
  a.guide = guide; a.gw = gw; a.gb = gb; a.partial = ws + pl.ws.at[WS_PARTIAL]; a.dy = dy;
  a.ksum = ws + pl.ws.at[pl.ksum]; a.kst = pl.kst; a.krow = pl.krow;
  a.P = pl.g.P; a.inv_ps = 1.0f / (float)pl.s.Ps; a.C = d->C; a.dzs = dz_stride; a.cq_n = pl.g.cq_n; a.rpi = pl.g.rpi;
  a.gw_stride = d->gw_stride; a.gw_coff = d->gw_coff; a.L = pl.g.L; a.plain = d->affine_only; a.sst = pl.g.sst;
  a.gw_ns = pl.gw_ns; a.gb_ns = pl.gb_ns; a.alpha = pl.alpha; a.keep = d->dropout_keep; a.seed = d->dropout_seed;
  a.post = pl.post ? 1 : 0;
  return a;
}

// src[K L][rows][C] (the reduce pass's partials, or pre_partials) -> sums[K][L][C] -> (L > 1) psum[K][C].  A simple plan's two
// totals are d beta / d gamma: the last launch writes them as well.
int bwd_sums(const NormPlan& pl, int C, const float* src, int rows, float* ws, float* dbeta, float* dgamma, hipStream_t st) {
  float *const al0 = pl.simple ? dbeta : nullptr, *const al1 = pl.simple ? dgamma : nullptr;
  const bool last1 = pl.g.L == 1;
  float* sums = ws + pl.ws.at[WS_SUMS];
  const int rc = unetk_rows_reduce_alias(src, pl.K * pl.g.L, rows, C, sums, ws + pl.ws.at[WS_TMP1], last1 ? al0 : nullptr,
                                         last1 ? al1 : nullptr, st);
  if (rc != UNETK_OK || last1) return rc;
  return unetk_rows_reduce_alias(sums, pl.K, pl.g.L, C, ws + pl.ws.at[WS_PSUM], ws + pl.ws.at[WS_TMP2], al0, al1, st);
}

}  // namespace

// bytes of the first part of the workspace (sums, first-level row sums), rounded up to 16: the refinement scratch follows
size_t finalize_ws_base(const unetk_norm_desc* d, const StatGeom& g, int stat_rows) {
  const size_t f = 2 * (size_t)g.Ns * d->C + unetk_rows_reduce_tmp_floats(2 * g.Ns, stat_rows / g.Ns, d->C);
  return (f * sizeof(float) + 15) / 16 * 16;
}

extern "C" size_t unetk_norm_finalize_ws_bytes(const unetk_norm_desc* d, int stat_rows) {
  if (!norm_desc_ok(d) || stat_rows <= 0) return 0;
  const StatGeom g = stat_geom(d);
  const size_t cblocks = (d->C + 15) / 16;
  // refinement (unetk_norm_finalize_y): part[Ns][cblocks][PB][2][16] and one[Ns][C][2] doubles, flags[Ns][C],
  // counters[Ns][cblocks]
  return finalize_ws_base(d, g, stat_rows) + (size_t)g.Ns * cblocks * refine_blocks(g.Ps) * 32 * sizeof(double) +
         (size_t)g.Ns * d->C * 2 * sizeof(double) + (size_t)g.Ns * d->C * sizeof(int) + (size_t)g.Ns * cblocks * sizeof(unsigned);
}

extern "C" int unetk_norm_finalize(const unetk_norm_desc* d, const float* stat_partials, int stat_rows,
                                   const float* gamma, const float* beta, float eps, float decay, int training,
                                   float* moving_mean, float* moving_var, float* mean_out, float* rstd_out,
                                   float* scale_out, float* shift_out, void* ws, size_t ws_bytes, void* stream) {
  return unetk_norm_finalize_y(d, stat_partials, stat_rows, nullptr, gamma, beta, eps, decay, training, moving_mean,
                               moving_var, mean_out, rstd_out, scale_out, shift_out, ws, ws_bytes, stream);
}

extern "C" int unetk_norm_finalize_y(const unetk_norm_desc* d, const float* stat_partials, int stat_rows, const float* y,
                                     const float* gamma, const float* beta, float eps, float decay, int training,
                                     float* moving_mean, float* moving_var, float* mean_out, float* rstd_out,
                                     float* scale_out, float* shift_out, void* ws, size_t ws_bytes, void* stream) {
  UNETK_REQUIRE(norm_desc_ok(d) && mean_out && rstd_out && scale_out && shift_out);
  hipStream_t st = (hipStream_t)stream;
  const StatGeom g = stat_geom(d);
  if (!d->per_sample && !training) {   // batch norm at inference: the moving statistics
    UNETK_REQUIRE(moving_mean && moving_var);
    UNETK_LAUNCH(norm_finalize_kernel, dim3((g.Ns * d->C + 255) / 256), dim3(256), 0, st, (const float*)nullptr, g.Ns, d->C,
                       (double)g.Ps, gamma, beta, eps, decay, 1, 0, moving_mean, moving_var, mean_out, rstd_out, scale_out,
                       shift_out);
    UNETK_LAUNCH_CHECK();
    return UNETK_OK;
  }
  UNETK_REQUIRE(stat_partials && stat_rows > 0 && ws && stat_rows % g.Ns == 0);
  UNETK_REQUIRE(!y || (d->storage == UNETK_FP32 && norm_supported(d) && unetk_aligned16(y) && unetk_aligned16(mean_out)));
  if (ws_bytes < unetk_norm_finalize_ws_bytes(d, stat_rows)) return UNETK_E_WORKSPACE;
  float* sums = (float*)ws;
  // partials are [2][stat_rows][C] with each image's tiles contiguous -> [2*Ns][rows_per_group][C]
  const float* src = stat_partials;
  int rows = stat_rows / g.Ns;
  if (rows > UNETK_RR_DIRECT_ROWS) {   // first level: 64 row blocks per (statistic, group)
    int rc = unetk_rows_reduce_l1(stat_partials, 2 * g.Ns, rows, d->C, sums + 2 * g.Ns * d->C, st);
    if (rc != UNETK_OK) return rc;
    src = sums + 2 * g.Ns * d->C;
    rows = 64;
  }
  const int update_moving = (!d->per_sample && training && moving_mean && moving_var) ? 1 : 0;
  const int cblocks = (d->C + 15) / 16, PB = refine_blocks(g.Ps);
  double* part = (double*)((char*)ws + finalize_ws_base(d, g, stat_rows));
  double* one = part + (size_t)g.Ns * cblocks * PB * 32;
  int* flags = y ? (int*)(one + (size_t)g.Ns * d->C * 2) : nullptr;
  unsigned* counters = y ? (unsigned*)(flags + (size_t)g.Ns * d->C) : nullptr;
  UNETK_LAUNCH(norm_reduce_finalize_kernel, dim3(cblocks * g.Ns), dim3(256), 0, st, src, rows, g.Ns, d->C, (double)g.Ps, gamma,
                     beta, eps, decay, update_moving, moving_mean, moving_var, mean_out, rstd_out, scale_out, shift_out, flags,
                     counters, one);
  UNETK_LAUNCH_CHECK();
  if (y) {
    UNETK_LAUNCH(norm_refine_kernel, dim3(PB * cblocks * g.Ns), dim3(256), 0, st, y, g.Ps, g.Ns, d->C, PB, (double)g.Ps, gamma,
                 beta, eps, decay, update_moving, moving_mean, moving_var, mean_out, rstd_out, scale_out, shift_out, flags,
                 counters, part, one);
    UNETK_LAUNCH_CHECK();
  }
  return UNETK_OK;
}

extern "C" int unetk_norm_apply_relu(const unetk_norm_desc* d, const void* y, const float* scale, const float* shift,
                                     const float* den, const float* guide, const float* gw, const float* gb, void* z,
                                     void* stream) {
  UNETK_REQUIRE(norm_desc_ok(d) && y && scale && shift && z && d->z_stride >= d->C);
  const NormPlan pl = norm_plan(d, NORM_APPLY, d->z_stride, 0, {den != nullptr, gb != nullptr, false, false, 0});
  if (!pl.shaped) return pl.rc;
  UNETK_REQUIRE(norm_storage_ok(d->storage, {y, z}) && unetk_aligned16(scale) && unetk_aligned16(shift));
  UNETK_REQUIRE((!den || unetk_aligned16(den)) && guide_operands_ok(d, guide, gw, gb));
  if (pl.rc != UNETK_OK) return pl.rc;
  const ApplyArgs a = apply_args(d, pl, y, scale, shift, den, guide, gw, gb, z);
  GD_DISPATCH(pl.bs, pl.G, pl.D, pl.leaky, norm_apply_relu_kernel, dim3(pl.gx, pl.g.L), dim3(256), 0, (hipStream_t)stream, a);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

// unetk_norm_apply_relu of a plain unit (no guide / density / dropout / post-shift) + unetk_maxpool2_fwd of its activation in one
// pass: z as there (pixel stride d->z_stride), pooled [N, H/2, W/2, C] dense.  d->HW = H * W, W given here, both even.
extern "C" int unetk_norm_apply_relu_pool(const unetk_norm_desc* d, int W, const void* y, const float* scale, const float* shift,
                                          void* z, void* pooled, void* stream) {
  UNETK_REQUIRE(norm_desc_ok(d) && y && scale && shift && z && pooled && d->z_stride >= d->C);
  const NormPlan pl = norm_plan(d, NORM_POOL_APPLY, d->z_stride, W, {});
  if (pl.rc != UNETK_OK) return pl.rc;
  UNETK_REQUIRE(norm_storage_ok(d->storage, {y, z, pooled}) && unetk_aligned16(scale) && unetk_aligned16(shift));
  const ApplyArgs a = apply_args(d, pl, y, scale, shift, nullptr, nullptr, nullptr, nullptr, z);
  T_DISPATCH(pl.bs, UNETK_LAUNCH(norm_apply_relu_pool_kernel<TT>, dim3(pl.gx, pl.g.L), dim3(256), 0, (hipStream_t)stream, a,
                                 pooled, d->HW / W, W, pl.g.L));
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" size_t unetk_norm_bwd_ws_bytes(const unetk_norm_desc* d) {
  if (!norm_desc_ok(d)) return 0;
  // planned with density and a gb block: no rule refuses BECAUSE one of them is there, so what this plan refuses, every plan of
  // the descriptor refuses -- and has no workspace.  Else one size for every variant: each segment as long as its longest, which
  // is K = 5 + G rows (density + leaky guide + post-shift row) over the density and the plain geometry.
  const NormPlan pl = norm_plan(d, NORM_BWD, d->C, 0, {true, true, true, false, 0});
  if (pl.rc != UNETK_OK) return 0;
  const int K = 5 + d->guide_ch;
  const LaunchGeom g1 = launch_geom(d, false);
  const NormWs a = bwd_ws_layout(K, pl.g.L, pl.nblk, d->C), b = bwd_ws_layout(K, g1.L, bwd_blocks(g1), d->C);
  size_t f = 0;
  for (int i = 0; i < WS_END; ++i) f += std::max(a.at[i + 1] - a.at[i], b.at[i + 1] - b.at[i]);
  return f * sizeof(float);
}

extern "C" int unetk_norm_relu_bwd(const unetk_norm_desc* d, const void* y, const void* dz, int dz_stride,
                                   const float* scale, const float* shift, const float* mean, const float* rstd,
                                   const float* den, const float* guide, const float* gw, const float* gb, void* dy,
                                   float* dgamma, float* dbeta, float* dden, float* dgw, float* dgb, void* ws,
                                   size_t ws_bytes, void* stream) {
  return unetk_norm_relu_bwd_pre(d, y, dz, dz_stride, scale, shift, mean, rstd, den, guide, gw, gb, dy, dgamma, dbeta, dden,
                                 dgw, dgb, nullptr, 0, ws, ws_bytes, stream);
}

// pre_partials [2][pre_rows][C] (nullable): the reduction pass's sums (sum du, sum du * xhat), per tile of the kernel that
// PRODUCED dz (unetk_conv3x3_dgrad_nbr) -- then only the apply pass runs here.  Plain units only (no guide, density,
// dropout, bias-only).
extern "C" int unetk_norm_relu_bwd_pre(const unetk_norm_desc* d, const void* y, const void* dz, int dz_stride,
                                       const float* scale, const float* shift, const float* mean, const float* rstd,
                                       const float* den, const float* guide, const float* gw, const float* gb, void* dy,
                                       float* dgamma, float* dbeta, float* dden, float* dgw, float* dgb,
                                       const float* pre_partials, int pre_rows, void* ws, size_t ws_bytes, void* stream) {
  UNETK_REQUIRE(norm_desc_ok(d) && y && dz && scale && shift && mean && rstd && dy && ws && dz_stride >= d->C);
  const NormPlan pl = norm_plan(d, NORM_BWD, dz_stride, 0,
                                {den != nullptr, gb != nullptr, dgb != nullptr, pre_partials != nullptr, pre_rows});
  if (!pl.shaped) return pl.rc;
  UNETK_REQUIRE(norm_storage_ok(d->storage, {y, dz, dy}) && unetk_aligned16(ws));
  UNETK_REQUIRE(!den || (dden && unetk_aligned16(den)));
  UNETK_REQUIRE(guide_operands_ok(d, guide, gw, gb) && (pl.G == 0 || dgw) && (!gb || dgb));
  if (ws_bytes < unetk_norm_bwd_ws_bytes(d)) return UNETK_E_WORKSPACE;
  if (pl.rc != UNETK_OK) return pl.rc;
  hipStream_t st = (hipStream_t)stream;
  float* const wsf = (float*)ws;
  const BwdArgs a = bwd_args(d, pl, wsf, y, dz, dz_stride, scale, shift, mean, rstd, den, guide, gw, gb, dy);
  const int G = pl.G;
  int rc = pre_partials ? bwd_sums(pl, d->C, pre_partials, pl.pre_rows, wsf, dbeta, dgamma, st) : UNETK_OK;
  if (!pre_partials) {
    if (pl.post) {
      T_DISPATCH(pl.bs, GL_DISPATCH(G, UNETK_LAUNCH((norm_bwd_reduce_kernel<GG, true, true, TT, true>), dim3(pl.nblk, pl.g.L),
                                                    dim3(256), pl.lds, st, a)));
    } else {
      GD_DISPATCH(pl.bs, G, pl.D, pl.leaky, norm_bwd_reduce_kernel, dim3(pl.nblk, pl.g.L), dim3(256), pl.lds, st, a);
    }
    UNETK_LAUNCH_CHECK();
    rc = bwd_sums(pl, d->C, a.partial, pl.nblk, wsf, dbeta, dgamma, st);
  }
  if (rc != UNETK_OK) return rc;
  const float *sums = wsf + pl.ws.at[WS_SUMS], *tot = wsf + pl.ws.at[pl.tot];
  if (!pl.simple) {
    UNETK_LAUNCH(norm_bwd_params_kernel, dim3((d->C + 255) / 256), dim3(256), 0, st, tot, d->C, pl.gps ? 0 : G,
                       (pl.D || pl.leaky) ? 1 : 0, dgamma, dbeta, pl.gps ? nullptr : dgw, (pl.gps || pl.post) ? nullptr : dgb);
    UNETK_LAUNCH_CHECK();
  }
  if (pl.gps) {   // dgw [N][G][C], dgb [N][C]: the per-launch-group sums, not their total
    UNETK_LAUNCH(norm_bwd_guide_ps_kernel, dim3((d->N * d->C + 255) / 256), dim3(256), 0, st, sums, d->N, d->C, G, pl.kb, dgw,
                       pl.post ? nullptr : dgb);
    UNETK_LAUNCH_CHECK();
  }
  if (pl.post) {  // gradient of the gb block: bias row = sum dg, slope rows = 0 (constants of the fold's sign), post-shift row = sum du
    UNETK_LAUNCH(norm_bwd_post_block_kernel, dim3((pl.groups * d->C + 255) / 256), dim3(256), 0, st, pl.gps ? sums : tot,
                       pl.groups, d->C, G, dgb);
    UNETK_LAUNCH_CHECK();
  }
  if (pl.D) {   // density gradient
    hipError_t e = hipMemcpyAsync(dden, wsf + pl.dden, (size_t)d->N * d->C * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return (int)e;
  }
  GD_DISPATCH(pl.bs, G, pl.D, pl.leaky, norm_bwd_apply_kernel, dim3(pl.gx, pl.g.L), dim3(256), 0, st, a);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

// The backward of a plain unit (no guide / density / dropout) whose output z feeds max_pool2d AND the skip connection:
// dz is never materialised.  dskip = the skip's gradient (pixel stride dskip_stride: a channel slice of the concat
// buffer's gradient), dp = the pooled tensor's gradient [N, H/2, W/2, C]; d->HW = H * W with W given here.
extern "C" int unetk_norm_relu_bwd_pool(const unetk_norm_desc* d, int W, const void* y, const void* dskip, int dskip_stride,
                                        const void* dp, const float* scale, const float* shift, const float* mean,
                                        const float* rstd, void* dy, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                                        void* stream) {
  UNETK_REQUIRE(norm_desc_ok(d) && y && dskip && dp && scale && shift && mean && rstd && dy && ws && dskip_stride >= d->C);
  const NormPlan pl = norm_plan(d, NORM_POOL_BWD, dskip_stride, W, {});
  if (pl.rc != UNETK_OK) return pl.rc;
  UNETK_REQUIRE(norm_storage_ok(d->storage, {y, dskip, dp, dy}) && unetk_aligned16(ws));
  if (ws_bytes < unetk_norm_bwd_ws_bytes(d)) return UNETK_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* const wsf = (float*)ws;
  const BwdArgs a = bwd_args(d, pl, wsf, y, dskip, dskip_stride, scale, shift, mean, rstd, nullptr, nullptr, nullptr, nullptr, dy);
  const PoolArgs pa{dp, d->HW / W, W};
  T_DISPATCH(pl.bs, UNETK_LAUNCH(norm_bwd_reduce_pool_kernel<TT>, dim3(pl.nblk, pl.g.L), dim3(256), pl.lds, st, a, pa));
  UNETK_LAUNCH_CHECK();
  const int rc = bwd_sums(pl, d->C, a.partial, pl.nblk, wsf, dbeta, dgamma, st);
  if (rc != UNETK_OK) return rc;
  T_DISPATCH(pl.bs, UNETK_LAUNCH(norm_bwd_apply_pool_kernel<TT>, dim3(pl.gx, pl.g.L), dim3(256), 0, st, a, pa));
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

// --use_se with --dropout, forward: sums [2][N][C] = per (sample, channel) sum of m * xhat and of m (see norm_drop_pool_kernel);
// d->dropout_keep / dropout_seed as in unetk_norm_apply_relu.  mean / rstd [groups][C] from unetk_norm_finalize.
extern "C" int unetk_norm_drop_pool(const unetk_norm_desc* d, const void* y, const float* mean, const float* rstd, float* sums,
                                    void* stream) {
  UNETK_REQUIRE(norm_desc_ok(d) && y && mean && rstd && sums);
  const NormPlan pl = norm_plan(d, NORM_DROP_POOL, d->C, 0, {});
  if (pl.rc != UNETK_OK) return pl.rc;
  UNETK_REQUIRE(norm_storage_ok(d->storage, {y}));
  T_DISPATCH(pl.bs, UNETK_LAUNCH(norm_drop_pool_kernel<TT>, dim3(d->N), dim3(256), pl.lds, (hipStream_t)stream, (const TT*)y, mean,
                                 rstd, sums, pl.g.P, d->C, pl.g.cq_n, pl.g.rpi, pl.g.sst, d->N, d->dropout_keep, d->dropout_seed));
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

// ... backward: dy += scale * (m E[b][c] - k1 - xhat k2); E [N][C], k1 / k2 [groups][C] (groups = N under instance norm, else 1).
extern "C" int unetk_norm_se_bwd_add_drop(const unetk_norm_desc* d, const void* y, void* dy, const float* mean, const float* rstd,
                                          const float* scale, const float* E, const float* k1, const float* k2, void* stream) {
  UNETK_REQUIRE(norm_desc_ok(d) && y && dy && mean && rstd && scale && E && k1 && k2);
  const NormPlan pl = norm_plan(d, NORM_SE_ADD_DROP, d->C, 0, {});
  if (pl.rc != UNETK_OK) return pl.rc;
  UNETK_REQUIRE(norm_storage_ok(d->storage, {y, dy}));
  UNETK_REQUIRE(unetk_aligned16(E) && unetk_aligned16(k1) && unetk_aligned16(k2) && unetk_aligned16(mean) && unetk_aligned16(rstd) &&
                unetk_aligned16(scale));
  T_DISPATCH(pl.bs, UNETK_LAUNCH(norm_se_bwd_add_drop_kernel<TT>, dim3(pl.gx, pl.g.L), dim3(256), 0, (hipStream_t)stream,
                                 (const TT*)y, (TT*)dy, mean, rstd, scale, E, k1, k2, pl.g.P, d->C, pl.g.cq_n, pl.g.rpi, pl.g.sst,
                                 d->dropout_keep, d->dropout_seed));
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_norm_se_bwd_add(const unetk_norm_desc* d, const void* y, void* dy, const float* mean, const float* rstd,
                                     const float* scale, const float* A, const float* k2, void* stream) {
  UNETK_REQUIRE(norm_desc_ok(d) && y && dy && mean && rstd && scale && A && k2);
  const NormPlan pl = norm_plan(d, NORM_SE_ADD, d->C, 0, {});      // one launch group per sample: A is per (sample, channel)
  if (pl.rc != UNETK_OK) return pl.rc;
  UNETK_REQUIRE(norm_storage_ok(d->storage, {y, dy}));
  UNETK_REQUIRE(unetk_aligned16(A) && unetk_aligned16(k2) && unetk_aligned16(mean) && unetk_aligned16(rstd) && unetk_aligned16(scale));
  T_DISPATCH(pl.bs, UNETK_LAUNCH(norm_se_bwd_add_kernel<TT>, dim3(pl.gx, pl.g.L), dim3(256), 0, (hipStream_t)stream, (const TT*)y,
                                 (TT*)dy, mean, rstd, scale, A, k2, pl.g.P, d->C, pl.g.cq_n, pl.g.rpi, pl.g.sst));
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}
