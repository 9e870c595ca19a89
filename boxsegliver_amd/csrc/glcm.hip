// Grey-level co-occurrence texture features of uint8 patches: the `glcm` context rows of GUNet.
// skimage's greycomatrix(levels=256, symmetric=True, normed=True) followed by the reference's greycoprops / glcm_features
// (utils/array_kits.py:1140-1232), one workgroup per (patch, offset).
//
// The symmetric matrix S = C + C^T is held as its upper triangle T[i][j >= i] in LDS: 32,896 uint32 = 131,584 B, so one
// workgroup per CU, which is why the workgroup is 16 waves wide.  A pair (a, b) adds 1 to T[min][max], 2 when a == b, by integer
// LDS atomics: the matrix is exact and independent of the order of the pixels.  The properties are fp64 sums over the triangle
// (off-diagonal entries weigh twice) in a fixed thread -> entry mapping, reduced by a fixed tree (wave butterflies, then the
// 16 wave partials in order): two runs give the same bits.  No floating-point atomics.
#include "common.h"

namespace {

constexpr int GL_LEVELS = 256;
constexpr int GL_TRI = GL_LEVELS * (GL_LEVELS + 1) / 2;          // 32,896
constexpr int GL_THREADS = 1024;
constexpr int GL_WAVES = GL_THREADS / 64;
constexpr int GL_NACC = 9;                                       // 7 plain sums + covariance + variance
constexpr int GL_MAX_K = 16;
constexpr int GL_MAX_EXTENT = 4096;
// T, the wave partials, {sum of i + j over the pairs (uint64), the reduced sums}
constexpr size_t GL_LDS_BYTES = (size_t)GL_TRI * 4 + (size_t)GL_WAVES * GL_NACC * 8 + 8 + GL_NACC * 8;

struct GlcmOffsets {
  int d[GL_MAX_K][2];
};

__device__ __forceinline__ int tri_index(int lo, int hi) { return lo * GL_LEVELS - ((lo * (lo - 1)) >> 1) + (hi - lo); }

__global__ __launch_bounds__(GL_THREADS) void glcm_kernel(const uint8_t* __restrict__ pix, const int32_t* __restrict__ patch_tab,
                                                          GlcmOffsets offs, int K, int norm_levels, double* __restrict__ out,
                                                          uint32_t* __restrict__ counts_out) {
  extern __shared__ __align__(16) unsigned char glcm_lds[];
  uint32_t* T = reinterpret_cast<uint32_t*>(glcm_lds);
  double* part = reinterpret_cast<double*>(glcm_lds + (size_t)GL_TRI * 4);
  unsigned long long* isum = reinterpret_cast<unsigned long long*>(part + GL_WAVES * GL_NACC);
  double* red = reinterpret_cast<double*>(isum + 1);

  const int p = blockIdx.x / K, k = blockIdx.x - p * K, tid = threadIdx.x;
  const int h = patch_tab[3 * p + 1], w = patch_tab[3 * p + 2];
  const uint8_t* img = pix + patch_tab[3 * p];
  const int dr = offs.d[k][0], dc = offs.d[k][1];

  for (int t = tid; t < GL_TRI; t += GL_THREADS) T[t] = 0u;
  if (tid == 0) *isum = 0ull;
  __syncthreads();

  // the pixels whose partner lies inside the patch: rows [r0, r0 + nr), columns [c0, c0 + nc)
  const int nr = h - abs(dr), nc = w - abs(dc);
  const int r0 = dr < 0 ? -dr : 0, c0 = dc < 0 ? -dc : 0;
  const int npairs = (nr > 0 && nc > 0) ? nr * nc : 0;
  unsigned long long mysum = 0ull;
  for (int idx = tid; idx < npairs; idx += GL_THREADS) {
    const int rr = idx / nc;
    const int r = r0 + rr, c = c0 + (idx - rr * nc);
    const int a = img[r * w + c], b = img[(r + dr) * w + (c + dc)];
    atomicAdd(&T[tri_index(min(a, b), max(a, b))], a == b ? 2u : 1u);
    mysum += (unsigned)(a + b);
  }
  if (mysum) atomicAdd(isum, mysum);
  __syncthreads();

  if (counts_out) {                                               // the full symmetric S, one writer per entry
    uint32_t* S = counts_out + ((size_t)p * K + k) * (GL_LEVELS * GL_LEVELS);
    for (int e = tid; e < GL_LEVELS * GL_LEVELS; e += GL_THREADS) {
      const int i = e >> 8, j = e & 255;
      S[e] = T[tri_index(min(i, j), max(i, j))];
    }
  }

  // sum(S) = 2 pairs; the mean of i (= the mean of j, S being symmetric) from the exact integer sum of i + j over the pairs
  const double total = npairs > 0 ? 2.0 * (double)npairs : 1.0;
  const double mean = (double)(*isum) / total;
  double acc[GL_NACC];
#pragma unroll
  for (int f = 0; f < GL_NACC; ++f) acc[f] = 0.0;
  for (int e = tid; e < GL_LEVELS * GL_LEVELS; e += GL_THREADS) {
    const int i = e >> 8, j = e & 255;
    if (j < i) continue;
    const uint32_t s = T[tri_index(i, j)];
    if (s == 0u) continue;
    const double P = (double)s / total;
    const double wgt = i == j ? P : 2.0 * P;
    const double d = (double)(i - j), d2 = d * d;
    const double di = (double)i - mean, dj = (double)j - mean, ds = di + dj;
    acc[0] += wgt * d2;
    acc[1] += wgt * fabs(d);
    acc[2] += wgt / (1.0 + d2);
    acc[3] += wgt * P;
    acc[4] += wgt * log(P + 1e-16);
    acc[5] += wgt * (di * dj);
    acc[6] += wgt * (ds * ds * ds);
    acc[7] += wgt * (ds * ds * ds * ds);
    acc[8] += i == j ? P * (di * di) : P * (di * di + dj * dj);
  }
#pragma unroll
  for (int f = 0; f < GL_NACC; ++f) acc[f] = wave_sum_d(acc[f]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int f = 0; f < GL_NACC; ++f) part[(tid >> 6) * GL_NACC + f] = acc[f];
  }
  __syncthreads();
  if (tid < GL_NACC) {
    double v = 0.0;
    for (int wv = 0; wv < GL_WAVES; ++wv) v += part[wv * GL_NACC + tid];
    red[tid] = v;
  }
  __syncthreads();
  if (tid == 0) {
    const double sd = sqrt(red[8]);
    double f[8];
    f[0] = red[0];
    f[1] = red[1];
    f[2] = red[2];
    f[3] = sqrt(red[3]);
    f[4] = -red[4];
    f[5] = sd < 1e-15 ? 1.0 : red[5] / (sd * sd);
    f[6] = red[6];
    f[7] = red[7];
    if (norm_levels) {                                            // glcm_features(norm_levels=True) for levels = 256
      f[0] /= 4096.0;
      f[1] /= 64.0;
      f[2] *= 2.0;
      f[3] *= 2.0;
      f[4] /= 8.0;
      f[6] /= 262144.0;
      f[7] /= 16777216.0;
    }
    for (int q = 0; q < 8; ++q) out[((size_t)p * 8 + q) * K + k] = f[q];
  }
}

inline size_t glcm_tab_bytes(int n) { return (((size_t)n * 3 * 4) + 15) & ~(size_t)15; }

}  // namespace

extern "C" size_t unetk_glcm_features_ws_bytes(int n, int K) {
  if (n < 1 || K < 1 || K > GL_MAX_K || n > (1 << 24)) return 0;
  return glcm_tab_bytes(n);
}

extern "C" int unetk_glcm_features(const uint8_t* pix, int64_t pix_bytes, const int32_t* patch_tab, int n, const int32_t* offsets,
                                   int K, int norm_levels, double* out, uint32_t* counts_out, void* ws, size_t ws_bytes,
                                   void* stream) {
  if (unetk_glcm_features_ws_bytes(n, K) == 0 || pix_bytes >= ((int64_t)1 << 31)) return UNETK_E_UNSUPPORTED;
  UNETK_REQUIRE(pix && patch_tab && offsets && out && ws && pix_bytes > 0);
  UNETK_REQUIRE((((uintptr_t)patch_tab) & 3u) == 0 && (((uintptr_t)offsets) & 3u) == 0 && unetk_aligned8(out) &&
                (((uintptr_t)counts_out) & 3u) == 0 && unetk_aligned16(ws));
  for (int p = 0; p < n; ++p) {
    const int h = patch_tab[3 * p + 1], w = patch_tab[3 * p + 2];
    if (h < 1 || h > GL_MAX_EXTENT || w < 1 || w > GL_MAX_EXTENT) return UNETK_E_UNSUPPORTED;
  }
  for (int p = 0; p < n; ++p) {
    const int64_t off = patch_tab[3 * p];
    UNETK_REQUIRE(off >= 0 && off + (int64_t)patch_tab[3 * p + 1] * patch_tab[3 * p + 2] <= pix_bytes);
  }
  if (ws_bytes < unetk_glcm_features_ws_bytes(n, K)) return UNETK_E_WORKSPACE;
  GlcmOffsets offs;
  for (int k = 0; k < GL_MAX_K; ++k) {
    for (int a = 0; a < 2; ++a) {
      // an offset beyond the largest extent pairs nothing in any patch: clamp it, so the kernel's index arithmetic stays small
      const int v = k < K ? offsets[2 * k + a] : 0;
      offs.d[k][a] = v > GL_MAX_EXTENT ? GL_MAX_EXTENT : (v < -GL_MAX_EXTENT ? -GL_MAX_EXTENT : v);
    }
  }
  hipStream_t st = (hipStream_t)stream;
  static bool attr_done = false;
  if (!attr_done) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(glcm_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)GL_LDS_BYTES);
    if (e != hipSuccess) return (int)e;
    attr_done = true;
  }
  // the table is the caller's host memory (it was validated above); the kernel reads the workspace copy
  const hipError_t e = hipMemcpyAsync(ws, patch_tab, (size_t)n * 3 * 4, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  UNETK_LAUNCH(glcm_kernel, dim3((unsigned)n * (unsigned)K), dim3(GL_THREADS), GL_LDS_BYTES, st, pix, (const int32_t*)ws, offs, K,
               norm_levels, out, counts_out);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}
