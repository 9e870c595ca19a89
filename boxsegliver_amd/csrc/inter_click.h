// What the two corrective-click steps share (inter_eval.hip: N slices per call; inter_eval3d.hip: one case
// per call; the shared core: 7.3.14).  Both work on a "region" of n elements -- a slice, i = y * W + x, or a
// case, i = (z * H + y) * W + x -- with an error byte, a label word and a size word per element, a header of 64-bit sums and
// keys and an info row of 32-bit results.  Shared: how an element's error bit, label and counts are set, the pick of the
// largest component, its coordinate means and the candidate, the row pass of the fallback's distance, and the fallback's
// arg-max with its key.  One copy, so the 2-D and the 3-D step cannot drift.  Each file keeps what is its own: which regions
// run (row states in 2-D, one case checked on the host in 3-D), where the prediction comes from, the sweep along z, the
// workspace layout, the finish kernel and its table row.  The components themselves come from unionfind.h.
#pragma once
#include "common.h"
#include "lits_clicks.h"     // CLK_MAX_EXTENT, clk_row_minplus
#include "unionfind.h"

namespace {

constexpr int IC_BLOCK = 256;
constexpr int IC_PER_THREAD = 8;         // elements a thread of the reducing kernels walks
constexpr int IC3_MAX_DEPTH = 4096;      // slices of a case

// Header and info slots.  The D coordinate sums and the D coordinates of the candidate are stored z first, so what follows
// them sits one slot lower in 2-D -- and HD_N with it, on which the workspace sizes depend.
enum { HD_NPRED = 0, HD_NREF, HD_NINTER, HD_NCOMP, HD_BEST, HD_SUM };
enum { IF_C = 0, IF_N = 8 };
template <int D>
struct IcSlots {
  enum { HD_FAR = HD_SUM + D, HD_N, IF_FALLBACK = D, IF_ROOT, IF_AREA };
};

// Per dimension: the type of a strided element index (a slice has at most 2^20 elements; a case has fewer than 2^31, but
// the last block's indices may pass that) and the field widths of the fallback's key below.
template <int D>
struct IcDim;
template <>
struct IcDim<2> {
  using Index = int;
  static constexpr int D2_BITS = 21, IDX_BITS = 20;
};
template <>
struct IcDim<3> {
  using Index = int64_t;
  static constexpr int D2_BITS = 25, IDX_BITS = 31;   // IDX_BITS: ic3_supported holds a case below 2^IDX_BITS voxels
};

// The fallback's arg-max key, high to low: the distance (a byte) | 2^D2_BITS - 1 - d2 | 2^IDX_BITS - 1 - i.  Under a max:
// the greater distance, then the smaller squared distance to the candidate, then the smaller linear index.
template <int D2_BITS, int IDX_BITS>
__device__ __forceinline__ unsigned long long ic_far_key(uint8_t dist, int d2, int i) {
  static_assert(8 + D2_BITS + IDX_BITS <= 64, "the key is one 64-bit word");
  return ((unsigned long long)dist << (D2_BITS + IDX_BITS)) | ((((1ull << D2_BITS) - 1) - (unsigned long long)d2) << IDX_BITS) |
         (((1ull << IDX_BITS) - 1) - (unsigned long long)i);
}
template <int D2_BITS, int IDX_BITS>
__device__ __forceinline__ int ic_far_index(unsigned long long key) {
  return (int)(((1ull << IDX_BITS) - 1) - (key & ((1ull << IDX_BITS) - 1)));
}
// the greatest squared distance between two voxels of a depth x CLK_MAX_EXTENT x CLK_MAX_EXTENT region
constexpr long long ic_max_d2(int depth) {
  return (long long)(depth - 1) * (depth - 1) + 2ll * (CLK_MAX_EXTENT - 1) * (CLK_MAX_EXTENT - 1);
}
static_assert(ic_max_d2(1) < (1ll << IcDim<2>::D2_BITS), "a slice's squared distances must fit the 2-D key");
static_assert((long long)CLK_MAX_EXTENT * CLK_MAX_EXTENT <= (1ll << IcDim<2>::IDX_BITS), "a slice's indices must fit the 2-D key");
static_assert(ic_max_d2(IC3_MAX_DEPTH) < (1ll << IcDim<3>::D2_BITS), "a case's squared distances must fit the 3-D key");

// ------------------------------------------------------------------------------------------------ indices and coordinates
template <int D>
__device__ __forceinline__ typename IcDim<D>::Index ic_strided(int u) {   // the u-th element of a reducing kernel's thread
  return (typename IcDim<D>::Index)blockIdx.x * (IC_BLOCK * IC_PER_THREAD) + u * IC_BLOCK + threadIdx.x;
}
template <int D>
__device__ __forceinline__ void ic_coords(int i, int W, int HW, int (&c)[D]) {   // (z,) y, x
  if constexpr (D == 3) {
    c[0] = i / HW;
    i -= c[0] * HW;
  }
  c[D - 2] = i / W;
  c[D - 1] = i - c[D - 2] * W;
}

// ------------------------------------------------------------------------------------------------ err, counts, label init
struct IcTally {
  unsigned long long np = 0, nr = 0, ni = 0;
};
// element i with prediction bit p and reference bit r: the error bit, a label of its own or none, no size yet
template <typename I>
__device__ __forceinline__ void ic_mark(IcTally& t, int p, int r, I i, uint8_t* __restrict__ err, int* __restrict__ label,
                                        int* __restrict__ cnt) {
  const int e = p ^ r;
  err[i] = (uint8_t)e;
  label[i] = e ? (int)i : -1;
  cnt[i] = 0;
  t.np += p;
  t.nr += r;
  t.ni += p & r;
}
__device__ __forceinline__ void ic_tally(const IcTally& t, unsigned long long* h) {
  const unsigned long long np = wave_sum(t.np), nr = wave_sum(t.nr), ni = wave_sum(t.ni);
  if ((threadIdx.x & 63) == 0) {
    if (np) atomicAdd(h + HD_NPRED, np);
    if (nr) atomicAdd(h + HD_NREF, nr);
    if (ni) atomicAdd(h + HD_NINTER, ni);
  }
}

// ------------------------------------------------------------------------------------------------ the largest component
// best = max over roots of (size, then the smaller root); the number of roots
template <int D>
__device__ __forceinline__ void ic_pick(const int* __restrict__ label, const int* __restrict__ cnt, typename IcDim<D>::Index n,
                                        unsigned long long* h) {
  unsigned long long key = 0ull, roots = 0ull;
#pragma unroll
  for (int u = 0; u < IC_PER_THREAD; ++u) {
    const auto i = ic_strided<D>(u);
    if (i < n && label[i] == (int)i) {
      const unsigned long long k = unetk_first_key((unsigned)cnt[i], (unsigned)i);
      key = k > key ? k : key;
      roots += 1;
    }
  }
  key = wave_max(key);
  roots = wave_sum(roots);
  if ((threadIdx.x & 63) == 0 && roots) {
    atomicMax(h + HD_BEST, key);
    atomicAdd(h + HD_NCOMP, roots);
  }
}

// the coordinate sums of the picked component
template <int D>
__device__ __forceinline__ void ic_mean(const int* __restrict__ label, typename IcDim<D>::Index n, int W, int HW,
                                        unsigned long long* h) {
  const unsigned long long best = h[HD_BEST];
  if (best == 0ull) return;                                  // no error element
  const int root = unetk_key_index(best);
  unsigned long long s[D] = {};
#pragma unroll
  for (int u = 0; u < IC_PER_THREAD; ++u) {
    const auto i = ic_strided<D>(u);
    if (i < n && label[i] == root) {
      int c[D];
      ic_coords<D>((int)i, W, HW, c);
#pragma unroll
      for (int k = 0; k < D; ++k) s[k] += (unsigned long long)c[k];
    }
  }
#pragma unroll
  for (int k = 0; k < D; ++k) s[k] = wave_sum(s[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < D; ++k)
      if (s[k]) atomicAdd(h + HD_SUM + k, s[k]);
  }
}

// One thread: the candidate = the component's mean per axis, rounded half to even (inside the region: a mean of its
// elements' coordinates); the fallback is due where err is not set there.  info stays zero without an error element.
template <int D>
__device__ __forceinline__ void ic_cand(const unsigned long long* h, int32_t* f, const uint8_t* __restrict__ err, int W, int HW) {
  using S = IcSlots<D>;
  const unsigned long long best = h[HD_BEST];
  if (best == 0ull) return;
  const unsigned long long area = best >> 32;
  int c[D];
#pragma unroll
  for (int k = 0; k < D; ++k) f[IF_C + k] = c[k] = unetk_round_div_even(h[HD_SUM + k], area);
  f[S::IF_ROOT] = unetk_key_index(best);
  f[S::IF_AREA] = (int)area;
  f[S::IF_FALLBACK] = err[(D == 3 ? (int64_t)c[0] * HW : 0) + (int64_t)c[D - 2] * W + c[D - 1]] ? 0 : 1;
}

// ------------------------------------------------------------------------------------------------ fallback
// One block, one row of cw elements: gf = the distance along the column (capped at `cap`), the region's border joins in,
// then the min-plus pass along the row.  gf <= cap, so every value the pass holds fits the byte.
__device__ __forceinline__ void ic_row_pass(int16_t (&buf)[2][1][CLK_MAX_EXTENT], const uint8_t* __restrict__ gf,
                                            uint8_t* __restrict__ dist, int cw, int cap) {
  for (int x = threadIdx.x; x < cw; x += IC_BLOCK) buf[0][0][x] = (int16_t)min((int)gf[x], min(x + 1, cw - x));
  __syncthreads();
  const int cur = clk_row_minplus<1>(buf, cw, cap);
  for (int x = threadIdx.x; x < cw; x += IC_BLOCK) dist[x] = (uint8_t)buf[cur][0][x];
}

// the arg-max of ic_far_key over the picked component
template <int D>
__device__ __forceinline__ void ic_far(const int* __restrict__ label, const uint8_t* __restrict__ dist, typename IcDim<D>::Index n,
                                       int W, int HW, const int32_t* f, unsigned long long* h) {
  using S = IcSlots<D>;
  if (f[S::IF_FALLBACK] == 0) return;
  const int root = f[S::IF_ROOT];
  int m[D];
#pragma unroll
  for (int k = 0; k < D; ++k) m[k] = f[IF_C + k];
  unsigned long long key = 0ull;
#pragma unroll
  for (int u = 0; u < IC_PER_THREAD; ++u) {
    const auto i = ic_strided<D>(u);
    if (i < n && label[i] == root) {
      int c[D], d2 = 0;
      ic_coords<D>((int)i, W, HW, c);
#pragma unroll
      for (int a = 0; a < D; ++a) d2 += (c[a] - m[a]) * (c[a] - m[a]);
      const unsigned long long k = ic_far_key<IcDim<D>::D2_BITS, IcDim<D>::IDX_BITS>(dist[i], d2, (int)i);
      key = k > key ? k : key;
    }
  }
  key = wave_max(key);
  if ((threadIdx.x & 63) == 0 && key) atomicMax(h + S::HD_FAR, key);
}

}  // namespace
