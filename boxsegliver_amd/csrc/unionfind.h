// The lock-free union-find that the component kernels share (evalvol.hip: 6- and 18-connected volumes; inter_eval.hip:
// 4-connected error regions of a slice; inter_eval3d.hip: 6-connected error regions of a case).  One copy, so the labellings
// cannot drift.
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

}  // namespace
