// The lock-free union-find that the component kernels share (evalvol.hip: 6- and 18-connected volumes; inter_eval.hip:
// 4-connected error regions of a slice; inter_eval3d.hip: 6-connected error regions of a case): find, union, the backward
// face unions and the flatten that leaves every element at its root.  One copy, so the labellings cannot drift.
#pragma once
#include "common.h"

namespace {

// Labels only ever decrease and every value a voxel has held names a member of its own set, so a stale read (an older
// parent, or a "root" that has since been linked) is still an ancestor: the union below stays correct and terminates, and
// the reads may come from the CU's own cache (workgroup scope) instead of all hitting the one L2 line of a big root.
__device__ __forceinline__ int ld_label(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// label[i] = -1 (background) or a voxel index <= i of the same component; roots have label[i] == i.  A union links the
// larger root under the smaller one with atomicMin (Playne & Hawick's lock-free union), so each tree's root is the minimum
// linear index of its component whatever order the atomics run in.
__device__ __forceinline__ int lc_find(const int* label, int p) {
  int q = ld_label(label + p);
  while (q != p) {
    p = q;
    q = ld_label(label + p);
  }
  return p;
}

__device__ __forceinline__ void lc_union(int* label, int a, int b) {
  for (;;) {
    a = lc_find(label, a);
    b = lc_find(label, b);
    if (a == b) return;
    if (a < b) {
      const int old = atomicMin(label + b, a);
      if (old == b) return;
      b = old;
    } else {
      const int old = atomicMin(label + a, b);
      if (old == a) return;
      a = old;
    }
  }
}

// 6-connectivity over a non-zero byte mask: element i = (z, y, x) of rows of W and planes of HW joins the up to three
// face neighbours that precede it in linear order; the other three are covered from their side.  z = 0 for a single plane.
__device__ __forceinline__ void lc_union_back6(const uint8_t* __restrict__ mask, int* label, int i, int x, int y, int z, int W,
                                               int HW) {
  if (x > 0 && mask[i - 1]) lc_union(label, i, i - 1);
  if (y > 0 && mask[i - W]) lc_union(label, i, i - W);
  if (z > 0 && mask[i - HW]) lc_union(label, i, i - HW);
}

// Element i of n points straight at its root r (-1: background, or i >= n).  Consecutive lanes are consecutive elements and
// mostly share a root: `lead` is the root of the wave's first lane (no lane's, if that one has none) and `same` the lanes
// that share it, so what they add at the root's slot can go in one atomic (a big component would otherwise take one per
// element on one address).  Every lane of the wave calls this.
struct LcFlat {
  int r, lead;
  unsigned long long same;
};
template <typename I>
__device__ __forceinline__ LcFlat lc_flatten(int* label, I i, I n) {
  LcFlat f;
  f.r = -1;
  if (i < n) {
    const int l = label[i];
    if (l >= 0) {
      f.r = lc_find(label, l);
      label[i] = f.r;
    }
  }
  f.lead = __builtin_amdgcn_readfirstlane(f.r >= 0 ? f.r : 0x7fffffff);
  f.same = __ballot(f.r == f.lead);
  return f;
}

// ... and component sizes at the roots' slots of `cnt`, by integer atomics
template <typename I>
__device__ __forceinline__ void lc_flatten_count(int* label, int* cnt, I i, I n) {
  const LcFlat f = lc_flatten(label, i, n);
  if (f.r < 0) return;
  if (f.r != f.lead)
    atomicAdd(cnt + f.r, 1);
  else if ((int)__lane_id() == __ffsll((long long)f.same) - 1)
    atomicAdd(cnt + f.r, __popcll(f.same));
}

}  // namespace
