// Volume evaluation on the device (evaluators/evaluator_liver.py _postprocess / _run_actual, loss_metrics.metric_3d):
// largest 6-connected component, the confusion counts, the 18-neighbourhood surface, the exact squared Euclidean distance
// transform and the surface-distance sums.  Masks are dense C-order uint8 [D,H,W], non-zero = object; D*H*W < 2^31, so a
// linear voxel index fits an int32.  Every reduction runs in a fixed order: results are bit-reproducible run to run.
#include "common.h"
#include "unionfind.h"   // lc_find, lc_union, lc_union_back6, lc_flatten: shared with inter_eval.hip and inter_eval3d.hip

namespace {

constexpr int EV_BLOCK = 256;
constexpr int EV_MAX_BLOCKS = 1024;          // fixed-grid reductions: partial rows per call (a function of the size only)

static inline int ev_blocks(int64_t n) { return (int)min((int64_t)EV_MAX_BLOCKS, max((int64_t)1, (n + EV_BLOCK * 8 - 1) / (EV_BLOCK * 8))); }
static inline int ev_grid1(int64_t n) { return (int)((n + EV_BLOCK - 1) / EV_BLOCK); }

static inline int ev_dims(int D, int H, int W) {
  if (D <= 0 || H <= 0 || W <= 0) return UNETK_E_BADARG;
  if ((int64_t)D * H * W >= ((int64_t)1 << 31)) return UNETK_E_UNSUPPORTED;
  return UNETK_OK;
}
static inline size_t ev_align(size_t b) { return (b + 255) & ~(size_t)255; }

// ---------------------------------------------------------------- largest 6-connected component (union-find)
// label[i] = -1 (background) or a voxel index <= i of the same component; roots have label[i] == i.  A union links the
// larger root under the smaller one with atomicMin (Playne & Hawick's lock-free union), so each tree's root is the minimum
// linear index of its component whatever order the atomics run in.
__global__ __launch_bounds__(EV_BLOCK) void lc_init_kernel(const uint8_t* __restrict__ mask, int n, int* __restrict__ label,
                                                           int* __restrict__ cnt, unsigned long long* __restrict__ best,
                                                           int32_t* __restrict__ info) {
  const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
  if (i == 0) *best = 0ull;
  if (i < 4) info[i] = 0;
  if (i >= n) return;
  label[i] = mask[i] ? i : -1;
  cnt[i] = 0;
}

__global__ __launch_bounds__(EV_BLOCK) void lc_merge_kernel(const uint8_t* __restrict__ mask, int D, int H, int W,
                                                            int* __restrict__ label) {
  const int n = D * H * W;
  const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
  if (i >= n || !mask[i]) return;
  lc_union_back6(mask, label, i, i % W, (i / W) % H, i / (H * W), W, H * W);
}

// every voxel points straight at its root; component sizes at the roots' slots
__global__ __launch_bounds__(EV_BLOCK) void lc_flatten_kernel(int n, int* __restrict__ label, int* __restrict__ cnt) {
  lc_flatten_count(label, cnt, (int)(blockIdx.x * EV_BLOCK + threadIdx.x), n);
}

// best = max over roots of (size << 32 | root): the largest component, the larger root (= scipy's larger label id) on ties
__global__ __launch_bounds__(EV_BLOCK) void lc_pick_kernel(int n, const int* __restrict__ label, const int* __restrict__ cnt,
                                                           unsigned long long* __restrict__ best) {
  __shared__ unsigned long long red[EV_BLOCK / 64];
  const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
  unsigned long long key = 0ull;
  if (i < n && label[i] == i) key = ((unsigned long long)(unsigned)cnt[i] << 32) | (unsigned)i;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long m = red[0];
#pragma unroll
    for (int j = 1; j < EV_BLOCK / 64; ++j) m = red[j] > m ? red[j] : m;
    if (m) atomicMax(best, m);
  }
}

// info[2] = number of components of the largest size, info[3] = number of components (wave-aggregated integer atomics)
__global__ __launch_bounds__(EV_BLOCK) void lc_ties_kernel(int n, const int* __restrict__ label, const int* __restrict__ cnt,
                                                           const unsigned long long* __restrict__ best,
                                                           int32_t* __restrict__ info) {
  const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
  const int top = (int)(*best >> 32);
  const bool root = i < n && label[i] == i;
  const unsigned long long roots = __ballot(root), ties = __ballot(root && cnt[i] == top);
  if ((threadIdx.x & 63) == 0) {
    if (roots) atomicAdd(info + 3, __popcll(roots));
    if (ties) atomicAdd(info + 2, __popcll(ties));
  }
}

// out = (label == root); root < 0 = the packed best's root (none for an empty mask); info[0..1] = {root, size}
__global__ __launch_bounds__(EV_BLOCK) void lc_write_kernel(int n, const int* __restrict__ label, const int* __restrict__ cnt,
                                                            const unsigned long long* __restrict__ best, int root,
                                                            uint8_t* __restrict__ out, int32_t* __restrict__ info) {
  const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
  if (root < 0) {
    const unsigned long long b = *best;
    root = b != 0ull ? (int)(unsigned)(b & 0xffffffffull) : -2;
  }
  if (i == 0 && info) {
    info[0] = root >= 0 ? root : -1;
    info[1] = root >= 0 ? cnt[root] : 0;
  }
  if (i >= n) return;
  out[i] = label[i] == root ? 1 : 0;
}

// ---------------------------------------------------------------- false-positive components (unetk_fp_mask3d)
// The mining rule of hard-negative training: the 6-connected components of pred >= pred_label that hold at
// least min_size voxels and share no voxel with the labelled object.  `out` serves as the 0/1 mask of the union-find first and
// is rewritten by fp_write_kernel; cnt[root] = the component's size, with FP_HIT set once a voxel of it lies on the object.
constexpr int FP_HIT = (int)0x80000000u;                   // a size is < 2^31: the sign bit is free

__global__ __launch_bounds__(EV_BLOCK) void fp_init_kernel(const uint8_t* __restrict__ pred, int n, int D, int pred_label,
                                                           uint8_t* __restrict__ mask, int* __restrict__ label,
                                                           int* __restrict__ cnt, int32_t* __restrict__ slice_counts,
                                                           int32_t* __restrict__ head) {
  const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
  if (i < 4) head[i] = 0;
  if (i < D) slice_counts[i] = 0;                            // D <= n
  if (i >= n) return;
  const bool m = (int)pred[i] >= pred_label;
  mask[i] = m ? 1 : 0;
  label[i] = m ? i : -1;
  cnt[i] = 0;
}

// after the flatten: a predicted voxel on the labelled object marks its root.  The flag only ever goes from clear to set, so the
// plain read that spares a big component its millions of atomics on one address cannot change the result.
__global__ __launch_bounds__(EV_BLOCK) void fp_overlap_kernel(const uint8_t* __restrict__ lab, int n, int thr,
                                                              const int* __restrict__ label, int* __restrict__ cnt) {
  const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int r = label[i];
  if (r < 0 || (int)lab[i] < thr) return;
  if (__hip_atomic_load(cnt + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0) atomicOr(cnt + r, FP_HIT);
}

// out, the per-slice counts and head = {components, kept components, kept voxels, 0}: integer atomics, one per wave and slice
// where the wave lies inside one slice (HW >= 64 mostly), else one per kept voxel
__global__ __launch_bounds__(EV_BLOCK) void fp_write_kernel(int n, int HW, const int* __restrict__ label,
                                                            const int* __restrict__ cnt, int min_size, int out_value,
                                                            uint8_t* __restrict__ out, int32_t* __restrict__ slice_counts,
                                                            int32_t* __restrict__ head) {
  const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
  const int r = i < n ? label[i] : -1;
  const int c = r >= 0 ? cnt[r] : 0;                         // negative with FP_HIT
  const bool kept = r >= 0 && c >= min_size;
  const bool root = r == i && i < n;
  if (i < n) out[i] = kept ? (uint8_t)out_value : 0;
  const unsigned long long mk = __ballot(kept), mr = __ballot(root), mkr = __ballot(root && kept);
  const int lane = threadIdx.x & 63;
  const int first = i - lane, last = min(first + 63, n - 1);
  const bool one_slice = first < n && first / HW == last / HW;   // wave-uniform
  if (one_slice) {
    if (lane == 0 && mk) atomicAdd(slice_counts + first / HW, __popcll(mk));
  } else if (kept) {
    atomicAdd(slice_counts + i / HW, 1);
  }
  if (lane == 0) {
    if (mr) atomicAdd(head + 0, __popcll(mr));
    if (mkr) atomicAdd(head + 1, __popcll(mkr));
    if (mk) atomicAdd(head + 2, __popcll(mk));
  }
}

// ---------------------------------------------------------------- counts |A|, |B|, |A and B|, |A or B|
__global__ __launch_bounds__(EV_BLOCK) void counts_partial_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                  int n, long long* __restrict__ part) {
  __shared__ long long red[4][EV_BLOCK];
  int ca = 0, cb = 0, ci = 0, cu = 0;
  for (int i = blockIdx.x * EV_BLOCK + threadIdx.x; i < n; i += gridDim.x * EV_BLOCK) {
    const int va = a[i] != 0, vb = b[i] != 0;
    ca += va; cb += vb; ci += va & vb; cu += va | vb;
  }
  red[0][threadIdx.x] = ca; red[1][threadIdx.x] = cb; red[2][threadIdx.x] = ci; red[3][threadIdx.x] = cu;
  __syncthreads();
  for (int s = EV_BLOCK / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s)
#pragma unroll
      for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x < 4) part[(int64_t)blockIdx.x * 4 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(EV_BLOCK) void counts_final_kernel(const long long* __restrict__ part, int rows,
                                                                long long* __restrict__ out) {
  __shared__ long long red[4][EV_BLOCK];
  long long s[4] = {0, 0, 0, 0};
  for (int r = threadIdx.x; r < rows; r += EV_BLOCK)
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += part[(int64_t)r * 4 + k];
#pragma unroll
  for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int h = EV_BLOCK / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h)
#pragma unroll
      for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x < 4) out[threadIdx.x] = red[threadIdx.x][0];
}

// ---------------------------------------------------------------- surface  A xor erode(A, 18-neighbourhood)
// box: {z0, y0, x0, z1, y1, x1}, half-open; atomicMin / atomicMax of per-block extents (order-free)
__global__ void box_init_kernel(int32_t* __restrict__ box) {
  if (threadIdx.x < 3) box[threadIdx.x] = 0x7fffffff;
  else if (threadIdx.x < 6) box[threadIdx.x] = 0;
}

__global__ __launch_bounds__(EV_BLOCK) void surface_kernel(const uint8_t* __restrict__ mask, int D, int H, int W,
                                                           uint8_t* __restrict__ edge, int32_t* __restrict__ box) {
  __shared__ int red[6][EV_BLOCK];
  const int n = D * H * W, HW = H * W;
  int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {0, 0, 0};
  for (int i = blockIdx.x * EV_BLOCK + threadIdx.x; i < n; i += gridDim.x * EV_BLOCK) {
    uint8_t e = 0;
    if (mask[i]) {
      const int x = i % W, y = (i / W) % H, z = i / HW;
      bool inner = x > 0 && x < W - 1 && y > 0 && y < H - 1 && z > 0 && z < D - 1;   // the border counts as background
      if (inner) {
        // 6 faces + 12 edges (generate_binary_structure(3, 2) without the centre)
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
          for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
              const int m = (dz != 0) + (dy != 0) + (dx != 0);
              if (m == 1 || m == 2) inner = inner && mask[i + dz * HW + dy * W + dx] != 0;
            }
      }
      if (!inner) {
        e = 1;
        lo[0] = min(lo[0], z); lo[1] = min(lo[1], y); lo[2] = min(lo[2], x);
        hi[0] = max(hi[0], z + 1); hi[1] = max(hi[1], y + 1); hi[2] = max(hi[2], x + 1);
      }
    }
    edge[i] = e;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { red[k][threadIdx.x] = lo[k]; red[3 + k][threadIdx.x] = hi[k]; }
  __syncthreads();
  for (int s = EV_BLOCK / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        red[k][threadIdx.x] = min(red[k][threadIdx.x], red[k][threadIdx.x + s]);
        red[3 + k][threadIdx.x] = max(red[3 + k][threadIdx.x], red[3 + k][threadIdx.x + s]);
      }
    __syncthreads();
  }
  if (threadIdx.x == 0 && red[3][0] > 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { atomicMin(box + k, red[k][0]); atomicMax(box + 3 + k, red[3 + k][0]); }
  }
}

// ---------------------------------------------------------------- exact squared EDT, one 1-D pass per launch
// One line per thread: f_out(q) = min_p f_in(p) + ((q - p) s)^2 over the line's part inside the box, by the lower envelope
// of parabolas (Felzenszwalb & Huttenlocher 2012).  Sites with f_in = +inf are left out; a line without a site is +inf.
// AXIS 2 (x) reads the feature mask (feature -> 0, else +inf), AXIS 1 / 0 the previous pass.  The envelope's site and
// boundary stacks live in the workspace at [k * nlines + line], so neighbouring threads touch neighbouring words.
template <int AXIS>
__global__ __launch_bounds__(EV_BLOCK) void edt_pass_kernel(const uint8_t* __restrict__ feat, const double* __restrict__ fin,
                                                            double* __restrict__ fout, int D, int H, int W,
                                                            const int32_t* __restrict__ box, double s,
                                                            int* __restrict__ vst, double* __restrict__ zst) {
  const int L = blockIdx.x * EV_BLOCK + threadIdx.x;
  const int nlines = AXIS == 2 ? D * H : (AXIS == 1 ? D * W : H * W);
  if (L >= nlines) return;
  const int z0 = max(box[0], 0), y0 = max(box[1], 0), x0 = max(box[2], 0);          // clamped: a box past the volume
  const int z1 = min(box[3], D), y1 = min(box[4], H), x1 = min(box[5], W);           // only shrinks to it
  int base, stride, lo, hi;
  if (AXIS == 2) {
    const int z = L / H, y = L % H;
    if (z < z0 || z >= z1 || y < y0 || y >= y1) return;
    base = (z * H + y) * W; stride = 1; lo = x0; hi = x1;
  } else if (AXIS == 1) {
    const int z = L / W, x = L % W;
    if (z < z0 || z >= z1 || x < x0 || x >= x1) return;
    base = z * H * W + x; stride = W; lo = y0; hi = y1;
  } else {
    const int y = L / W, x = L % W;
    if (y < y0 || y >= y1 || x < x0 || x >= x1) return;
    base = L; stride = H * W; lo = z0; hi = z1;
  }
  const double INF = __builtin_huge_val();
  const double ss2 = 2.0 * s * s;
  int k = -1;
  for (int q = lo; q < hi; ++q) {
    const int iq = base + q * stride;
    const double fq = AXIS == 2 ? (feat[iq] ? 0.0 : INF) : fin[iq];
    if (fq == INF) continue;
    const double cq = (double)(q - lo) * s;
    double zq = -INF;
    while (k >= 0) {
      const int p = vst[(int64_t)k * nlines + L];
      const double fp = AXIS == 2 ? 0.0 : fin[base + p * stride];
      const double cp = (double)(p - lo) * s;
      const double sx = ((fq + cq * cq) - (fp + cp * cp)) / (ss2 * (double)(q - p));   // intersection, in index units - lo
      if (sx <= zst[(int64_t)k * nlines + L]) {
        --k;
      } else {
        zq = sx;
        break;
      }
    }
    ++k;
    vst[(int64_t)k * nlines + L] = q;
    zst[(int64_t)k * nlines + L] = zq;
  }
  if (k < 0) {
    for (int q = lo; q < hi; ++q) fout[base + q * stride] = INF;
    return;
  }
  const int kmax = k;
  k = 0;
  int p = vst[L];
  double fp = AXIS == 2 ? 0.0 : fin[base + p * stride];
  for (int q = lo; q < hi; ++q) {
    while (k < kmax && zst[(int64_t)(k + 1) * nlines + L] < (double)(q - lo)) {
      ++k;
      p = vst[(int64_t)k * nlines + L];
      fp = AXIS == 2 ? 0.0 : fin[base + p * stride];
    }
    const double d = (double)(q - p) * s;
    fout[base + q * stride] = d * d + fp;
  }
}

// ---------------------------------------------------------------- surface distance sums
// over the voxels of `surf`: d = sqrt(dist2); sum d, sum d*d, max d, count -- fixed-order per-block partials, one final block
__global__ __launch_bounds__(EV_BLOCK) void sdist_partial_kernel(const uint8_t* __restrict__ surf, const double* __restrict__ dist2,
                                                                 int n, double* __restrict__ part) {
  __shared__ double red[4][EV_BLOCK];
  double s1 = 0.0, s2 = 0.0, mx = 0.0;
  int c = 0;
  for (int i = blockIdx.x * EV_BLOCK + threadIdx.x; i < n; i += gridDim.x * EV_BLOCK) {
    if (surf[i]) {
      const double d = sqrt(dist2[i]);
      s1 += d; s2 += d * d; mx = fmax(mx, d); ++c;
    }
  }
  red[0][threadIdx.x] = s1; red[1][threadIdx.x] = s2; red[2][threadIdx.x] = mx; red[3][threadIdx.x] = (double)c;
  __syncthreads();
  for (int h = EV_BLOCK / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) {
      red[0][threadIdx.x] += red[0][threadIdx.x + h];
      red[1][threadIdx.x] += red[1][threadIdx.x + h];
      red[2][threadIdx.x] = fmax(red[2][threadIdx.x], red[2][threadIdx.x + h]);
      red[3][threadIdx.x] += red[3][threadIdx.x + h];                 // integers < 2^31: exact in fp64
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) part[(int64_t)blockIdx.x * 4 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(EV_BLOCK) void sdist_final_kernel(const double* __restrict__ part, int rows, double* __restrict__ out) {
  __shared__ double red[4][EV_BLOCK];
  double s1 = 0.0, s2 = 0.0, mx = 0.0, c = 0.0;
  for (int r = threadIdx.x; r < rows; r += EV_BLOCK) {
    s1 += part[(int64_t)r * 4 + 0];
    s2 += part[(int64_t)r * 4 + 1];
    mx = fmax(mx, part[(int64_t)r * 4 + 2]);
    c += part[(int64_t)r * 4 + 3];
  }
  red[0][threadIdx.x] = s1; red[1][threadIdx.x] = s2; red[2][threadIdx.x] = mx; red[3][threadIdx.x] = c;
  __syncthreads();
  for (int h = EV_BLOCK / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) {
      red[0][threadIdx.x] += red[0][threadIdx.x + h];
      red[1][threadIdx.x] += red[1][threadIdx.x + h];
      red[2][threadIdx.x] = fmax(red[2][threadIdx.x], red[2][threadIdx.x + h]);
      red[3][threadIdx.x] += red[3][threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = red[0][0];
    out[1] = red[1][0];
    out[2] = red[2][0];
    reinterpret_cast<long long*>(out)[3] = (long long)red[3][0];
  }
}

// ---------------------------------------------------------------- per-slice HU histograms (the context guide's feature rows)
// Every count is an integer atomic (LDS per block, then global), so the counts do not depend on the order the atomics run
// in; the densities are then one correctly rounded fp64 division chain per bin, as numpy computes them.
constexpr int SH_MAX_BINS = 1024;

// bin of an HU value through the host's lookup table (numpy's edge rule already applied); -1 = not counted
__device__ __forceinline__ int sh_bin(int v, const int32_t* __restrict__ lut, int lut_lo, int lut_n) {
  const int d = v - lut_lo;
  return (unsigned)d < (unsigned)lut_n ? lut[d] : -1;
}

__global__ __launch_bounds__(EV_BLOCK) void sh_zero_kernel(int32_t* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * EV_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * EV_BLOCK) p[i] = 0;
}

// grid (blocks per slice, D): counts[k][0, bins) over labels >= 1; with TRAIN also counts[k][bins, 2 bins) over labels == 2
template <bool TRAIN>
__global__ __launch_bounds__(EV_BLOCK) void sh_slice_kernel(const int16_t* __restrict__ vol, const uint8_t* __restrict__ lab,
                                                            int HW, const int32_t* __restrict__ lut, int lut_lo, int lut_n,
                                                            int bins, int32_t* __restrict__ counts) {
  extern __shared__ int sh_hist[];
  const int nh = TRAIN ? 2 * bins : bins;
  for (int j = threadIdx.x; j < nh; j += EV_BLOCK) sh_hist[j] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.y * HW;
  for (int i = blockIdx.x * EV_BLOCK + threadIdx.x; i < HW; i += gridDim.x * EV_BLOCK) {
    const int l = lab[base + i];
    if (l == 0) continue;
    const int b = sh_bin(vol[base + i], lut, lut_lo, lut_n);
    if (b < 0) continue;
    atomicAdd(sh_hist + b, 1);
    if (TRAIN && l == 2) atomicAdd(sh_hist + bins + b, 1);
  }
  __syncthreads();
  int32_t* row = counts + (int64_t)blockIdx.y * 2 * bins;
  for (int j = threadIdx.x; j < nh; j += EV_BLOCK)
    if (sh_hist[j]) atomicAdd(row + j, sh_hist[j]);
}

// eval mode: the tumour voxels (label == 2) as union-find roots of their own; zmax = last slice of a root's component
__global__ __launch_bounds__(EV_BLOCK) void sh_label_init_kernel(const uint8_t* __restrict__ lab, int n, int* __restrict__ label,
                                                                 int* __restrict__ zmax) {
  const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
  if (i >= n) return;
  label[i] = lab[i] == 2 ? i : -1;
  zmax[i] = -1;
}

// 18-connectivity (ndi.generate_binary_structure(3, 2)): the 9 face and edge neighbours that precede a voxel in linear
// order; the other 9 are covered from their side
__global__ __launch_bounds__(EV_BLOCK) void sh_merge18_kernel(const uint8_t* __restrict__ lab, int D, int H, int W,
                                                              int* __restrict__ label) {
  const int n = D * H * W, HW = H * W;
  const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
  if (i >= n || lab[i] != 2) return;
  const int x = i % W, y = (i / W) % H, z = i / HW;
  if (x > 0 && lab[i - 1] == 2) lc_union(label, i, i - 1);
  if (y > 0) {
    if (lab[i - W] == 2) lc_union(label, i, i - W);
    if (x > 0 && lab[i - W - 1] == 2) lc_union(label, i, i - W - 1);
    if (x < W - 1 && lab[i - W + 1] == 2) lc_union(label, i, i - W + 1);
  }
  if (z > 0) {
    const int j = i - HW;
    if (lab[j] == 2) lc_union(label, i, j);
    if (y > 0 && lab[j - W] == 2) lc_union(label, i, j - W);
    if (y < H - 1 && lab[j + W] == 2) lc_union(label, i, j + W);
    if (x > 0 && lab[j - 1] == 2) lc_union(label, i, j - 1);
    if (x < W - 1 && lab[j + 1] == 2) lc_union(label, i, j + 1);
  }
}

// every voxel points straight at its root (the component's minimum linear index, so its first slice is root / HW); the
// last slice by atomicMax at the root, one per wave for the lanes that share the wave's first root (their highest lane
// holds their largest z: consecutive lanes are consecutive voxels)
__global__ __launch_bounds__(EV_BLOCK) void sh_flatten_kernel(int n, int HW, int* __restrict__ label, int* __restrict__ zmax) {
  const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
  const LcFlat f = lc_flatten(label, i, n);
  if (f.r < 0) return;
  if (f.r != f.lead || (int)__lane_id() == 63 - __clzll((long long)f.same)) atomicMax(zmax + f.r, i / HW);
}

// array_kits.guide_pixel_list(middle, tile_guide): the voxels of component c on its middle slice m add their bins to
// every row of c's extent [z0, z1) -- as a difference array over z: +1 at z0, -1 at z1 (diff has D + 1 rows)
__global__ __launch_bounds__(EV_BLOCK) void sh_mid_kernel(const int16_t* __restrict__ vol, int n, int HW,
                                                          const int* __restrict__ label, const int* __restrict__ zmax,
                                                          const int32_t* __restrict__ lut, int lut_lo, int lut_n, int bins,
                                                          int32_t* __restrict__ diff) {
  const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int r = label[i];
  if (r < 0) return;
  const int z0 = r / HW, z1 = zmax[r] + 1;
  if (i / HW != (z1 - z0 - 1) / 2 + z0) return;
  const int b = sh_bin(vol[i], lut, lut_lo, lut_n);
  if (b < 0) return;
  atomicAdd(diff + (int64_t)z0 * bins + b, 1);
  atomicAdd(diff + (int64_t)z1 * bins + b, -1);
}

// counts[k][bins + b] = prefix sum of diff[0..k][b]: one thread per bin, rows in order
__global__ __launch_bounds__(EV_BLOCK) void sh_prefix_kernel(const int32_t* __restrict__ diff, int D, int bins,
                                                             int32_t* __restrict__ counts) {
  const int b = blockIdx.x * EV_BLOCK + threadIdx.x;
  if (b >= bins) return;
  int run = 0;
  for (int k = 0; k < D; ++k) {
    run += diff[(int64_t)k * bins + b];
    counts[(int64_t)k * 2 * bins + bins + b] = run;
  }
}

// one block per row: np.histogram(density=True) = (count / db) / total in fp64, rounded to fp32; an empty half is 0
// (nan_to_num of 0 / 0)
__global__ __launch_bounds__(EV_BLOCK) void sh_density_kernel(const int32_t* __restrict__ counts, const double* __restrict__ db,
                                                              int bins, float* __restrict__ out) {
  __shared__ long long red[2][EV_BLOCK];
  const int32_t* row = counts + (int64_t)blockIdx.x * 2 * bins;
  long long s0 = 0, s1 = 0;
  for (int j = threadIdx.x; j < bins; j += EV_BLOCK) {
    s0 += row[j];
    s1 += row[bins + j];
  }
  red[0][threadIdx.x] = s0;
  red[1][threadIdx.x] = s1;
  __syncthreads();
  for (int h = EV_BLOCK / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) {
      red[0][threadIdx.x] += red[0][threadIdx.x + h];
      red[1][threadIdx.x] += red[1][threadIdx.x + h];
    }
    __syncthreads();
  }
  const long long t0 = red[0][0], t1 = red[1][0];
  float* o = out + (int64_t)blockIdx.x * 2 * bins;
  for (int j = threadIdx.x; j < 2 * bins; j += EV_BLOCK) {
    const long long t = j < bins ? t0 : t1;
    const int b = j < bins ? j : j - bins;
    o[j] = t > 0 ? (float)(((double)row[j] / db[b]) / (double)t) : 0.f;
  }
}

// ---------------------------------------------------------------- guide propagation: tumour components of one slice
// (DataLoader/Liver/input_pipeline_g.py:1246-1318, the `last_pred` setter of EvalImage3DLoader).  The tumour mask is
// argmax(acc) == 2 (lowest index on ties, as head_predict_kernel); its 4-connected components are the labels of
// lc_init / lc_merge / lc_flatten run with D = 1.  Roots are numbered in increasing linear index (scipy's label order) by
// one block; per component integer atomics fill a row and a column histogram and a packed (guide value, -index) max; one
// thread per component then reads its box, the exact medians and the median absolute deviations off the histograms.
constexpr int GC_ROW = 12;            // int32 words per table row (include/unetk.h)
constexpr int GC_ENUM = 1024;         // threads of the numbering block

__global__ __launch_bounds__(EV_BLOCK) void gc_mask_kernel(const float* __restrict__ acc, int n, uint8_t* __restrict__ mask) {
  const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float a0 = acc[3 * (int64_t)i], a1 = acc[3 * (int64_t)i + 1], a2 = acc[3 * (int64_t)i + 2];
  const float b = a1 > a0 ? a1 : a0;          // strict comparisons: the first index wins ties (np.argmax)
  mask[i] = a2 > b ? 1 : 0;
}

// cid[root] = rank of the root among all roots (scipy's label - 1); rows [0, cap) get {root, area}; head = {count, overflow}.
// One block walks the image in tiles of GC_ENUM consecutive pixels (coalesced reads): a ballot per wave, the waves' counts
// in LDS, so each root's rank is the roots before its tile + before its wave + before its lane -- increasing linear order.
__global__ __launch_bounds__(GC_ENUM) void gc_enum_kernel(int n, const int* __restrict__ label, const int* __restrict__ cnt,
                                                          int cap, int* __restrict__ cid, int32_t* __restrict__ table) {
  __shared__ int wsum[GC_ENUM / 64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  int base = 0;                                  // roots in the tiles before this one (the same in every thread)
  for (int i0 = 0; i0 < n; i0 += GC_ENUM) {
    const int i = i0 + t;
    const bool root = i < n && label[i] == i;
    const unsigned long long b = __ballot(root);
    if (lane == 0) wsum[wv] = __popcll(b);
    __syncthreads();
    int before = base, total = base;
    for (int j = 0; j < GC_ENUM / 64; ++j) {
      const int c = wsum[j];
      before += j < wv ? c : 0;
      total += c;
    }
    __syncthreads();                             // wsum is rewritten by the next tile
    if (root) {
      const int k = before + __popcll(b & ((1ull << lane) - 1ull));
      cid[i] = k;
      if (k < cap) {
        table[4 + (int64_t)k * GC_ROW] = i;
        table[4 + (int64_t)k * GC_ROW + 1] = cnt[i];
      }
    }
    base = total;
  }
  if (t == 0) {
    table[0] = base;
    table[1] = base > cap ? 1 : 0;
    table[2] = 0;
    table[3] = 0;
  }
}

// zero the histograms and the peak key of the components that exist: a fixed grid strides over min(count, cap)
constexpr int GC_ZERO_BLOCKS = 256;
__global__ __launch_bounds__(EV_BLOCK) void gc_zero_kernel(const int32_t* __restrict__ table, int cap, int H, int W,
                                                           int* __restrict__ hrow, int* __restrict__ hcol,
                                                           unsigned long long* __restrict__ peak) {
  const int count = min(table[0], cap);
  for (int k = blockIdx.x; k < count; k += gridDim.x) {
    for (int j = threadIdx.x; j < H; j += EV_BLOCK) hrow[(int64_t)k * H + j] = 0;
    for (int j = threadIdx.x; j < W; j += EV_BLOCK) hcol[(int64_t)k * W + j] = 0;
    if (threadIdx.x == 0) peak[k] = 0ull;
  }
}

__device__ __forceinline__ unsigned int gc_order_bits(float g) {     // float -> unsigned key with the same order
  const unsigned int u = __float_as_uint(g);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float gc_order_float(unsigned int k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// per pixel of a component: row / column histogram counts and the packed max (guide value, then the smaller index); the
// lanes that share the wave's first (component, row) add once for all of them, as lc_flatten does for the sizes
__global__ __launch_bounds__(EV_BLOCK) void gc_accum_kernel(int n, int H, int W, const int* __restrict__ label,
                                                            const int* __restrict__ cid, const float* __restrict__ guide,
                                                            int cap, int* __restrict__ hrow, int* __restrict__ hcol,
                                                            unsigned long long* __restrict__ peak) {
  const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
  int k = -1, y = 0, x = 0;
  unsigned long long key = 0ull;
  if (i < n) {
    const int r = label[i];
    if (r >= 0) {
      const int c = cid[r];
      if (c < cap) {
        k = c;
        y = i / W;
        x = i - y * W;
        key = unetk_first_key(gc_order_bits(guide[i]), (unsigned int)i);
      }
    }
  }
  const int ry = k >= 0 ? k * H + y : 0x7fffffff;   // < cap * H < 2^31 (unetk_guide_components checks it)
  const int lead = __builtin_amdgcn_readfirstlane(ry);
  const unsigned long long same = __ballot(k >= 0 && ry == lead);
  const int kl = __builtin_amdgcn_readfirstlane(k >= 0 ? k : 0x7fffffff);
  const bool in_lead = k >= 0 && k == kl;
  const unsigned long long m = wave_max(in_lead ? key : 0ull);
  const int first = __ffsll((long long)__ballot(in_lead)) - 1;
  if (k < 0) return;
  if (ry != lead)
    atomicAdd(hrow + ry, 1);
  else if ((int)__lane_id() == __ffsll((long long)same) - 1)
    atomicAdd(hrow + ry, __popcll(same));
  atomicAdd(hcol + (int64_t)k * W + x, 1);
  if (!in_lead)
    atomicMax(peak + k, key);
  else if ((int)__lane_id() == first)
    atomicMax(peak + k, m);
}

// the bin of the p-th smallest value (0-based) of a histogram over [lo, hi]
__device__ __forceinline__ int gc_select(const int* __restrict__ h, int lo, int hi, int p) {
  int acc = 0;
  for (int r = lo; r <= hi; ++r) {
    acc += h[r];
    if (acc > p) return r;
  }
  return hi;
}

// median and 1.4826 x median absolute deviation of the values a histogram holds, as array_kits.compute_robust_moments
// computes them in float32: twice the median c2 is an integer, and so is twice each distance |2 r - c2| / 2, walked outward
__device__ __forceinline__ void gc_moments(const int* __restrict__ h, int lo, int hi, int cnt, float* ctr, float* std) {
  const int c2 = gc_select(h, lo, hi, (cnt - 1) / 2) + gc_select(h, lo, hi, cnt / 2);
  const int pa = (cnt - 1) / 2, pb = cnt / 2;
  int da = -1, db = -1, acc = 0;
  for (int d2 = c2 & 1; db < 0; d2 += 2) {
    const int ra = (c2 - d2) / 2, rb = (c2 + d2) / 2;
    int c = 0;
    if (ra >= lo && ra <= hi) c += h[ra];
    if (d2 > 0 && rb >= lo && rb <= hi) c += h[rb];
    if (da < 0 && acc + c > pa) da = d2;
    if (acc + c > pb) db = d2;
    acc += c;
    if (d2 > 2 * (hi - lo) + 2) {            // cannot happen for a consistent histogram; keeps the loop finite
      if (da < 0) da = d2;
      db = d2;
    }
  }
  *ctr = (float)c2 * 0.5f;
  const float mad = ((float)da * 0.5f + (float)db * 0.5f) / 2.f;
  *std = 1.4826f * mad;
}

__global__ __launch_bounds__(EV_BLOCK) void gc_final_kernel(int H, int W, int cap, const int* __restrict__ hrow,
                                                            const int* __restrict__ hcol,
                                                            const unsigned long long* __restrict__ peak,
                                                            int32_t* __restrict__ table) {
  const int k = blockIdx.x * EV_BLOCK + threadIdx.x;
  if (k >= min(table[0], cap)) return;
  int32_t* row = table + 4 + (int64_t)k * GC_ROW;
  const int area = row[1];
  const int* hr = hrow + (int64_t)k * H;
  const int* hc = hcol + (int64_t)k * W;
  int y0 = 0, y1 = H - 1, x0 = 0, x1 = W - 1;
  while (y0 < H - 1 && hr[y0] == 0) ++y0;
  while (y1 > y0 && hr[y1] == 0) --y1;
  while (x0 < W - 1 && hc[x0] == 0) ++x0;
  while (x1 > x0 && hc[x1] == 0) --x1;
  float cy, cx, sy, sx;
  gc_moments(hr, y0, y1, area, &cy, &sy);
  gc_moments(hc, x0, x1, area, &cx, &sx);
  const unsigned long long p = peak[k];
  row[2] = y0;
  row[3] = x0;
  row[4] = y1;
  row[5] = x1;
  row[6] = unetk_key_index(p);
  row[7] = __float_as_int(gc_order_float((unsigned int)(p >> 32)));
  row[8] = __float_as_int(cy);
  row[9] = __float_as_int(cx);
  row[10] = __float_as_int(sy);
  row[11] = __float_as_int(sx);
}

// ---------------------------------------------------------------- component overlaps of two masks (per-lesion detection)
// utils/array_kits.py:883-984 distinct_binary_object_correspondences asks, per reference object, which result objects it
// shares voxels with and how many.  Both masks are labelled by lc_init / lc_merge / lc_flatten; roots are numbered in
// increasing linear index over tiles of CO_TILE voxels (count, scan, write); the pairs are keyed by their two roots
// (reference root high, result root low: the order of the keys is the order of the (ref_id, res_id) pairs), made distinct
// in an open-addressing table of n slots, ranked among themselves, and counted per voxel against the ranked list.  Every
// value written is an integer that no order of the atomics changes.
constexpr int CO_TILE = EV_BLOCK * 16;       // voxels per block of the numbering kernels
constexpr int CO_SCAN = 1024;                // threads of the tile-count scan
constexpr int CO_MAX_CAP = 1 << 24;          // cap_obj, cap_pair: row indices times the row width stay far inside an int
constexpr unsigned long long CO_EMPTY = ~0ull;   // no key: roots are < 2^31

static inline int co_tiles(int64_t n) { return (int)((n + CO_TILE - 1) / CO_TILE); }

__global__ __launch_bounds__(EV_BLOCK) void co_fill_kernel(unsigned long long* __restrict__ p, int64_t n, unsigned long long v) {
  for (int64_t i = (int64_t)blockIdx.x * EV_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * EV_BLOCK) p[i] = v;
}

// tsum[m * nt + b] = number of roots of mask m (blockIdx.y) in tile b
__global__ __launch_bounds__(EV_BLOCK) void co_tile_roots_kernel(int n, const int* __restrict__ label0,
                                                                 const int* __restrict__ label1, int nt, int* __restrict__ tsum) {
  __shared__ int red[EV_BLOCK / 64];
  const int* label = blockIdx.y ? label1 : label0;
  const int64_t base = (int64_t)blockIdx.x * CO_TILE;
  int c = 0;
  for (int j = 0; j < CO_TILE / EV_BLOCK; ++j) {
    const int64_t i = base + j * EV_BLOCK + threadIdx.x;
    c += (i < n && label[i] == (int)i) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int j = 0; j < EV_BLOCK / 64; ++j) s += red[j];
    tsum[(int64_t)blockIdx.y * nt + blockIdx.x] = s;
  }
}

// one block per mask: tsum -> its exclusive prefix sums; head[m] = number of components, head[3] bit m = more than cap_obj
__global__ __launch_bounds__(CO_SCAN) void co_scan_kernel(int nt, int* __restrict__ tsum, int cap_obj, int32_t* __restrict__ table) {
  __shared__ int part[CO_SCAN];
  int* s = tsum + (int64_t)blockIdx.x * nt;
  const int t = threadIdx.x;
  const int per = (nt + CO_SCAN - 1) / CO_SCAN;
  const int lo = min(nt, t * per), hi = min(nt, lo + per);
  int sum = 0;
  for (int k = lo; k < hi; ++k) sum += s[k];
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < CO_SCAN; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - sum;
  for (int k = lo; k < hi; ++k) {
    const int c = s[k];
    s[k] = run;
    run += c;
  }
  if (t == CO_SCAN - 1) {
    table[blockIdx.x] = part[t];
    if (part[t] > cap_obj) atomicOr(table + 3, 1 << blockIdx.x);
  }
}

// rows {root, size} of mask m (blockIdx.y) for the roots of rank < cap_obj: rank = roots in the tiles before (tsum) +
// before this pass of the tile + before this wave + before this lane, as gc_enum_kernel ranks them
__global__ __launch_bounds__(EV_BLOCK) void co_rows_kernel(int n, const int* __restrict__ label0, const int* __restrict__ label1,
                                                           const int* __restrict__ cnt0, const int* __restrict__ cnt1, int nt,
                                                           const int* __restrict__ tsum, int cap_obj, int32_t* __restrict__ table) {
  __shared__ int wsum[EV_BLOCK / 64];
  const int* label = blockIdx.y ? label1 : label0;
  const int* cnt = blockIdx.y ? cnt1 : cnt0;
  int32_t* rows = table + 4 + (int64_t)blockIdx.y * 2 * cap_obj;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t first = (int64_t)blockIdx.x * CO_TILE;
  int base = tsum[(int64_t)blockIdx.y * nt + blockIdx.x];
  for (int j = 0; j < CO_TILE / EV_BLOCK; ++j) {
    const int64_t i = first + j * EV_BLOCK + threadIdx.x;
    const bool root = i < n && label[i] == (int)i;
    const unsigned long long b = __ballot(root);
    if (lane == 0) wsum[wv] = __popcll(b);
    __syncthreads();
    int before = base, total = base;
#pragma unroll
    for (int q = 0; q < EV_BLOCK / 64; ++q) {
      const int c = wsum[q];
      before += q < wv ? c : 0;
      total += c;
    }
    __syncthreads();                             // wsum is rewritten by the next pass
    if (root) {
      const int k = before + __popcll(b & ((1ull << lane) - 1ull));
      if (k < cap_obj) {
        rows[2 * (int64_t)k] = (int)i;
        rows[2 * (int64_t)k + 1] = cnt[i];
      }
    }
    base = total;
  }
}

__device__ __forceinline__ int co_slot(unsigned long long k, int n) {          // murmur3's 64-bit finaliser, then [0, n)
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (int)(((k & 0xffffffffull) * (unsigned long long)(unsigned)n) >> 32);
}

// The key of voxel i, CO_EMPTY outside the overlap.
__device__ __forceinline__ unsigned long long co_key(int64_t i, int n, const int* __restrict__ lres, const int* __restrict__ lref) {
  if (i >= n) return CO_EMPTY;
  const int a = lref[i], b = lres[i];
  return a >= 0 && b >= 0 ? ((unsigned long long)(unsigned)a << 32) | (unsigned)b : CO_EMPTY;
}

// Calls f(key, lanes holding it) once per distinct key of the wave, in the first lane that holds it: a whole lesion is one
// key, so a wave inside it makes one table access, not 64 on one address.  Every lane of the wave must call this.
template <class F>
__device__ __forceinline__ void co_per_key(unsigned long long key, F f) {
  unsigned long long todo = __ballot(key != CO_EMPTY);
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1;
    const unsigned long long k = __shfl(key, lead);
    const unsigned long long same = __ballot(key == k);
    if ((int)__lane_id() == lead) f(k, __popcll(same));
    todo &= ~same;
  }
}

// keys -> the table of n slots, each distinct key once.  Two face neighbours of the overlap share both components, so the
// distinct pairs are at most ceil(n / 2): a free slot is always found; the probe count is bounded all the same.
__global__ __launch_bounds__(EV_BLOCK) void co_insert_kernel(int n, const int* __restrict__ lres, const int* __restrict__ lref,
                                                             unsigned long long* __restrict__ slots) {
  const unsigned long long key = co_key((int64_t)blockIdx.x * EV_BLOCK + threadIdx.x, n, lres, lref);
  co_per_key(key, [&](unsigned long long k, int) {
    int s = co_slot(k, n);
    for (int probe = 0; probe < n; ++probe) {
      const unsigned long long cur = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == k) return;
      if (cur == CO_EMPTY) {
        const unsigned long long old = atomicCAS(slots + s, CO_EMPTY, k);
        if (old == CO_EMPTY || old == k) return;
      }
      s = s + 1 == n ? 0 : s + 1;
    }
  });
}

// the used slots -> list (any order, the first cap_pair of them); head[2] = their number
__global__ __launch_bounds__(EV_BLOCK) void co_compact_kernel(int n, const unsigned long long* __restrict__ slots, int cap_pair,
                                                              unsigned long long* __restrict__ list, int32_t* __restrict__ table) {
  const int lane = threadIdx.x & 63;
  for (int64_t i0 = (int64_t)blockIdx.x * EV_BLOCK; i0 < n; i0 += (int64_t)gridDim.x * EV_BLOCK) {
    const int64_t i = i0 + threadIdx.x;
    const unsigned long long k = i < n ? slots[i] : CO_EMPTY;
    const unsigned long long b = __ballot(k != CO_EMPTY);
    if (b == 0ull) continue;
    const int lead = __ffsll((long long)b) - 1;
    int at = 0;
    if (lane == lead) at = atomicAdd(table + 2, __popcll(b));
    at = __shfl(at, lead) + __popcll(b & ((1ull << lane) - 1ull));
    if (k != CO_EMPTY && at < cap_pair) list[at] = k;
  }
}

// the pair rows are written only when nothing overflowed: which cap_pair keys the list kept depends on the atomics
__device__ __forceinline__ int co_listed(const int32_t* __restrict__ table, int cap_obj, int cap_pair) {
  return table[0] > cap_obj || table[1] > cap_obj || table[2] > cap_pair ? 0 : table[2];
}

// rows[2 * j] over j in [0, count) ascending: the 1-based rank of `root`
__device__ __forceinline__ int co_id(const int32_t* __restrict__ rows, int count, int root) {
  int lo = 0, hi = count;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rows[2 * (int64_t)mid] < root) lo = mid + 1; else hi = mid;
  }
  return lo + 1;
}

// rank of every listed key among them (keys are distinct): sorted[rank] = key and pair row rank = {ref_id, res_id, 0};
// head[3] bit 2 = more than cap_pair pairs
__global__ __launch_bounds__(EV_BLOCK) void co_rank_kernel(const unsigned long long* __restrict__ list, int cap_obj, int cap_pair,
                                                           unsigned long long* __restrict__ sorted, int32_t* __restrict__ table) {
  __shared__ unsigned long long tile[EV_BLOCK];
  if (blockIdx.x == 0 && threadIdx.x == 0 && table[2] > cap_pair) atomicOr(table + 3, 4);
  const int m = co_listed(table, cap_obj, cap_pair);
  if ((int64_t)blockIdx.x * EV_BLOCK >= m) return;
  const int g = blockIdx.x * EV_BLOCK + threadIdx.x;
  const unsigned long long key = g < m ? list[g] : CO_EMPTY;
  int rank = 0;
  for (int t0 = 0; t0 < m; t0 += EV_BLOCK) {
    const int j = t0 + threadIdx.x;
    tile[threadIdx.x] = j < m ? list[j] : CO_EMPTY;
    __syncthreads();
    const int cnt = min(EV_BLOCK, m - t0);
    for (int q = 0; q < cnt; ++q) rank += tile[q] < key ? 1 : 0;
    __syncthreads();
  }
  if (g >= m) return;
  sorted[rank] = key;
  const int32_t* res_rows = table + 4;
  const int32_t* ref_rows = table + 4 + 2 * (int64_t)cap_obj;
  int32_t* row = table + 4 + 4 * (int64_t)cap_obj + 3 * (int64_t)rank;
  row[0] = co_id(ref_rows, table[1], (int)(key >> 32));
  row[1] = co_id(res_rows, table[0], (int)(key & 0xffffffffull));
}

// overlap of every listed pair: one add of the lane count per distinct key of a wave, at the key's place in the sorted list
__global__ __launch_bounds__(EV_BLOCK) void co_count_kernel(int n, const int* __restrict__ lres, const int* __restrict__ lref,
                                                            const unsigned long long* __restrict__ sorted, int cap_obj,
                                                            int cap_pair, int32_t* __restrict__ table) {
  const int m = co_listed(table, cap_obj, cap_pair);
  if (m == 0) return;
  const unsigned long long key = co_key((int64_t)blockIdx.x * EV_BLOCK + threadIdx.x, n, lres, lref);
  int32_t* pairs = table + 4 + 4 * (int64_t)cap_obj;
  co_per_key(key, [&](unsigned long long k, int lanes) {
    int lo = 0, hi = m;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (sorted[mid] < k) lo = mid + 1; else hi = mid;
    }
    if (lo < m && sorted[lo] == k) atomicAdd(pairs + 3 * (int64_t)lo + 2, lanes);
  });
}

}  // namespace

// ---------------------------------------------------------------- C ABI
extern "C" size_t unetk_largest_component_ws_bytes(int D, int H, int W) {
  if (ev_dims(D, H, W) != UNETK_OK) return 0;
  return 2 * ev_align((size_t)D * H * W * 4) + 256;
}

extern "C" int unetk_largest_component(const uint8_t* mask, int D, int H, int W, uint8_t* out, int32_t* info, void* ws,
                                       size_t ws_bytes, void* stream) {
  const int dims = ev_dims(D, H, W);
  if (dims != UNETK_OK) return dims;
  UNETK_REQUIRE(mask && out && info && ws && unetk_aligned16(ws) && (((uintptr_t)info) & 3u) == 0);
  if (ws_bytes < unetk_largest_component_ws_bytes(D, H, W)) return UNETK_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int n = D * H * W;
  int* label = (int*)ws;
  int* cnt = (int*)((char*)ws + ev_align((size_t)n * 4));
  unsigned long long* best = (unsigned long long*)((char*)ws + 2 * ev_align((size_t)n * 4));
  const int g = ev_grid1(n);
  UNETK_LAUNCH(lc_init_kernel, dim3(g), dim3(EV_BLOCK), 0, st, mask, n, label, cnt, best, info);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(lc_merge_kernel, dim3(g), dim3(EV_BLOCK), 0, st, mask, D, H, W, label);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(lc_flatten_kernel, dim3(g), dim3(EV_BLOCK), 0, st, n, label, cnt);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(lc_pick_kernel, dim3(g), dim3(EV_BLOCK), 0, st, n, (const int*)label, (const int*)cnt, best);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(lc_ties_kernel, dim3(g), dim3(EV_BLOCK), 0, st, n, (const int*)label, (const int*)cnt,
               (const unsigned long long*)best, info);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(lc_write_kernel, dim3(g), dim3(EV_BLOCK), 0, st, n, (const int*)label, (const int*)cnt,
               (const unsigned long long*)best, -1, out, info);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_component_mask(const void* ws, int D, int H, int W, int32_t root, uint8_t* out, void* stream) {
  const int dims = ev_dims(D, H, W);
  if (dims != UNETK_OK) return dims;
  UNETK_REQUIRE(ws && out && unetk_aligned16(ws) && root >= 0 && (int64_t)root < (int64_t)D * H * W);
  hipStream_t st = (hipStream_t)stream;
  const int n = D * H * W;
  const int* label = (const int*)ws;
  const int* cnt = (const int*)((const char*)ws + ev_align((size_t)n * 4));
  UNETK_LAUNCH(lc_write_kernel, dim3(ev_grid1(n)), dim3(EV_BLOCK), 0, st, n, label, cnt, (const unsigned long long*)nullptr, root,
               out, (int32_t*)nullptr);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" size_t unetk_fp_mask3d_ws_bytes(int D, int H, int W) {
  if (ev_dims(D, H, W) != UNETK_OK) return 0;
  return 2 * ev_align((size_t)D * H * W * 4);
}

extern "C" int unetk_fp_mask3d(const uint8_t* pred, const uint8_t* lab, int D, int H, int W, int pred_label, int lab_scale,
                               int obj_label, int min_size, int out_value, uint8_t* out, int32_t* slice_counts, int32_t* head,
                               void* ws, size_t ws_bytes, void* stream) {
  const int dims = ev_dims(D, H, W);
  if (dims != UNETK_OK) return dims;
  UNETK_REQUIRE(pred && lab && out && slice_counts && head && ws && unetk_aligned16(ws));
  UNETK_REQUIRE(((((uintptr_t)slice_counts) | ((uintptr_t)head)) & 3u) == 0);
  UNETK_REQUIRE(pred_label >= 1 && lab_scale >= 1 && obj_label >= 1 && (int64_t)lab_scale * obj_label < ((int64_t)1 << 31) &&
                min_size >= 1 && out_value >= 1 && out_value <= 255);
  if (ws_bytes < unetk_fp_mask3d_ws_bytes(D, H, W)) return UNETK_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int n = D * H * W;
  int* label = (int*)ws;
  int* cnt = (int*)((char*)ws + ev_align((size_t)n * 4));
  const int g = ev_grid1(n);
  UNETK_LAUNCH(fp_init_kernel, dim3(g), dim3(EV_BLOCK), 0, st, pred, n, D, pred_label, out, label, cnt, slice_counts, head);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(lc_merge_kernel, dim3(g), dim3(EV_BLOCK), 0, st, (const uint8_t*)out, D, H, W, label);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(lc_flatten_kernel, dim3(g), dim3(EV_BLOCK), 0, st, n, label, cnt);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(fp_overlap_kernel, dim3(g), dim3(EV_BLOCK), 0, st, lab, n, lab_scale * obj_label, (const int*)label, cnt);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(fp_write_kernel, dim3(g), dim3(EV_BLOCK), 0, st, n, H * W, (const int*)label, (const int*)cnt, min_size, out_value,
               out, slice_counts, head);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" size_t unetk_mask_counts_ws_bytes(int D, int H, int W) {
  if (ev_dims(D, H, W) != UNETK_OK) return 0;
  return (size_t)ev_blocks((int64_t)D * H * W) * 4 * 8;
}

extern "C" int unetk_mask_counts(const uint8_t* a, const uint8_t* b, int D, int H, int W, int64_t* counts, void* ws,
                                 size_t ws_bytes, void* stream) {
  const int dims = ev_dims(D, H, W);
  if (dims != UNETK_OK) return dims;
  UNETK_REQUIRE(a && b && counts && ws && unetk_aligned16(ws) && unetk_aligned8(counts));
  if (ws_bytes < unetk_mask_counts_ws_bytes(D, H, W)) return UNETK_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int n = D * H * W, rows = ev_blocks(n);
  UNETK_LAUNCH(counts_partial_kernel, dim3(rows), dim3(EV_BLOCK), 0, st, a, b, n, (long long*)ws);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(counts_final_kernel, dim3(1), dim3(EV_BLOCK), 0, st, (const long long*)ws, rows, (long long*)counts);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_surface3d(const uint8_t* mask, int D, int H, int W, uint8_t* edge, int32_t* box, int accumulate_box,
                               void* stream) {
  const int dims = ev_dims(D, H, W);
  if (dims != UNETK_OK) return dims;
  UNETK_REQUIRE(mask && edge && box && (((uintptr_t)box) & 3u) == 0);
  hipStream_t st = (hipStream_t)stream;
  if (!accumulate_box) {
    UNETK_LAUNCH(box_init_kernel, dim3(1), dim3(64), 0, st, box);
    UNETK_LAUNCH_CHECK();
  }
  const int n = D * H * W;
  UNETK_LAUNCH(surface_kernel, dim3(ev_blocks(n)), dim3(EV_BLOCK), 0, st, mask, D, H, W, edge, box);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" size_t unetk_edt3d_sq_ws_bytes(int D, int H, int W) {
  if (ev_dims(D, H, W) != UNETK_OK) return 0;
  const size_t n = (size_t)D * H * W;
  return 2 * ev_align(n * 8) + ev_align(n * 4);
}

extern "C" int unetk_edt3d_sq(const uint8_t* feature, int D, int H, int W, const int32_t* box, double sz, double sy, double sx,
                              double* dist2, void* ws, size_t ws_bytes, void* stream) {
  const int dims = ev_dims(D, H, W);
  if (dims != UNETK_OK) return dims;
  UNETK_REQUIRE(feature && box && dist2 && ws && unetk_aligned16(ws) && unetk_aligned8(dist2) && (((uintptr_t)box) & 3u) == 0);
  UNETK_REQUIRE(sz > 0.0 && sy > 0.0 && sx > 0.0);
  if (ws_bytes < unetk_edt3d_sq_ws_bytes(D, H, W)) return UNETK_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)D * H * W;
  double* tmp = (double*)ws;
  double* zst = (double*)((char*)ws + ev_align(n * 8));
  int* vst = (int*)((char*)ws + 2 * ev_align(n * 8));
  UNETK_LAUNCH(edt_pass_kernel<2>, dim3(ev_grid1((int64_t)D * H)), dim3(EV_BLOCK), 0, st, feature, (const double*)nullptr, dist2,
               D, H, W, box, sx, vst, zst);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(edt_pass_kernel<1>, dim3(ev_grid1((int64_t)D * W)), dim3(EV_BLOCK), 0, st, feature, (const double*)dist2, tmp,
               D, H, W, box, sy, vst, zst);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(edt_pass_kernel<0>, dim3(ev_grid1((int64_t)H * W)), dim3(EV_BLOCK), 0, st, feature, (const double*)tmp, dist2,
               D, H, W, box, sz, vst, zst);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" size_t unetk_surface_dist_ws_bytes(int D, int H, int W) {
  if (ev_dims(D, H, W) != UNETK_OK) return 0;
  return (size_t)ev_blocks((int64_t)D * H * W) * 4 * 8;
}

extern "C" int unetk_surface_dist(const uint8_t* surf, const double* dist2, int D, int H, int W, double* out, void* ws,
                                  size_t ws_bytes, void* stream) {
  const int dims = ev_dims(D, H, W);
  if (dims != UNETK_OK) return dims;
  UNETK_REQUIRE(surf && dist2 && out && ws && unetk_aligned16(ws) && unetk_aligned8(out) && unetk_aligned8(dist2));
  if (ws_bytes < unetk_surface_dist_ws_bytes(D, H, W)) return UNETK_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int n = D * H * W, rows = ev_blocks(n);
  UNETK_LAUNCH(sdist_partial_kernel, dim3(rows), dim3(EV_BLOCK), 0, st, surf, dist2, n, (double*)ws);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(sdist_final_kernel, dim3(1), dim3(EV_BLOCK), 0, st, (const double*)ws, rows, out);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

static inline size_t sh_counts_bytes(int D, int bins) { return ev_align((size_t)D * 2 * bins * 4); }

extern "C" size_t unetk_slice_hist_ws_bytes(int D, int H, int W, int bins, int mode) {
  if (ev_dims(D, H, W) != UNETK_OK || bins <= 0 || bins > SH_MAX_BINS || (mode != 0 && mode != 1)) return 0;
  size_t b = sh_counts_bytes(D, bins);
  if (mode == 1) b += 2 * ev_align((size_t)D * H * W * 4) + ev_align((size_t)(D + 1) * bins * 4);
  return b;
}

extern "C" int unetk_slice_hist(const int16_t* vol, const uint8_t* lab, int D, int H, int W, int mode, const int32_t* lut,
                                int lut_lo, int lut_n, const double* db, int bins, float* out, void* ws, size_t ws_bytes,
                                void* stream) {
  const int dims = ev_dims(D, H, W);
  if (dims != UNETK_OK) return dims;
  UNETK_REQUIRE(vol && lab && lut && db && out && ws && unetk_aligned16(ws) && unetk_aligned8(db));
  UNETK_REQUIRE((((uintptr_t)vol) & 1u) == 0 && (((uintptr_t)lut) & 3u) == 0 && (((uintptr_t)out) & 3u) == 0);
  UNETK_REQUIRE((mode == 0 || mode == 1) && bins > 0 && bins <= SH_MAX_BINS && lut_n > 0);
  if (ws_bytes < unetk_slice_hist_ws_bytes(D, H, W, bins, mode)) return UNETK_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int n = D * H * W, HW = H * W;
  int32_t* counts = (int32_t*)ws;
  const int64_t ncounts = (int64_t)D * 2 * bins;
  UNETK_LAUNCH(sh_zero_kernel, dim3(ev_blocks(ncounts)), dim3(EV_BLOCK), 0, st, counts, ncounts);
  UNETK_LAUNCH_CHECK();
  const dim3 sgrid((unsigned)min(64, max(1, (HW + EV_BLOCK * 16 - 1) / (EV_BLOCK * 16))), (unsigned)D);
  if (mode == 0) {
    UNETK_LAUNCH(sh_slice_kernel<true>, sgrid, dim3(EV_BLOCK), 2 * bins * 4, st, vol, lab, HW, lut, lut_lo, lut_n, bins, counts);
    UNETK_LAUNCH_CHECK();
  } else {
    char* p = (char*)ws + sh_counts_bytes(D, bins);
    int* label = (int*)p;
    int* zmax = (int*)(p + ev_align((size_t)n * 4));
    int32_t* diff = (int32_t*)(p + 2 * ev_align((size_t)n * 4));
    const int64_t ndiff = (int64_t)(D + 1) * bins;
    const int g = ev_grid1(n);
    UNETK_LAUNCH(sh_slice_kernel<false>, sgrid, dim3(EV_BLOCK), bins * 4, st, vol, lab, HW, lut, lut_lo, lut_n, bins, counts);
    UNETK_LAUNCH_CHECK();
    UNETK_LAUNCH(sh_zero_kernel, dim3(ev_blocks(ndiff)), dim3(EV_BLOCK), 0, st, diff, ndiff);
    UNETK_LAUNCH_CHECK();
    UNETK_LAUNCH(sh_label_init_kernel, dim3(g), dim3(EV_BLOCK), 0, st, lab, n, label, zmax);
    UNETK_LAUNCH_CHECK();
    UNETK_LAUNCH(sh_merge18_kernel, dim3(g), dim3(EV_BLOCK), 0, st, lab, D, H, W, label);
    UNETK_LAUNCH_CHECK();
    UNETK_LAUNCH(sh_flatten_kernel, dim3(g), dim3(EV_BLOCK), 0, st, n, HW, label, zmax);
    UNETK_LAUNCH_CHECK();
    UNETK_LAUNCH(sh_mid_kernel, dim3(g), dim3(EV_BLOCK), 0, st, vol, n, HW, (const int*)label, (const int*)zmax, lut, lut_lo,
                 lut_n, bins, diff);
    UNETK_LAUNCH_CHECK();
    UNETK_LAUNCH(sh_prefix_kernel, dim3((bins + EV_BLOCK - 1) / EV_BLOCK), dim3(EV_BLOCK), 0, st, (const int32_t*)diff, D, bins,
                 counts);
    UNETK_LAUNCH_CHECK();
  }
  UNETK_LAUNCH(sh_density_kernel, dim3(D), dim3(EV_BLOCK), 0, st, (const int32_t*)counts, db, bins, out);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

// ---------------------------------------------------------------- guide propagation
static inline size_t gc_n_bytes(int H, int W) { return ev_align((size_t)H * W * 4); }

extern "C" size_t unetk_guide_components_ws_bytes(int H, int W, int cap) {
  if (ev_dims(1, H, W) != UNETK_OK || cap <= 0 || cap > (1 << 16)) return 0;
  if ((int64_t)cap * H >= ((int64_t)1 << 31) || (int64_t)cap * W >= ((int64_t)1 << 31)) return 0;
  const size_t nb = gc_n_bytes(H, W);
  return 3 * nb + ev_align((size_t)H * W) + 256 + ev_align((size_t)cap * H * 4) + ev_align((size_t)cap * W * 4) +
         ev_align((size_t)cap * 8);
}

extern "C" int unetk_guide_components(const float* acc, const float* guide, int H, int W, int cap, int32_t* table, void* ws,
                                      size_t ws_bytes, void* stream) {
  const int dims = ev_dims(1, H, W);
  if (dims != UNETK_OK) return dims;
  UNETK_REQUIRE(acc && guide && table && ws && unetk_aligned16(ws) && cap > 0 && cap <= (1 << 16));
  UNETK_REQUIRE((int64_t)cap * H < ((int64_t)1 << 31) && (int64_t)cap * W < ((int64_t)1 << 31));    // int histogram indices
  UNETK_REQUIRE((((uintptr_t)table) & 3u) == 0 && (((uintptr_t)acc) & 3u) == 0 && (((uintptr_t)guide) & 3u) == 0);
  if (ws_bytes < unetk_guide_components_ws_bytes(H, W, cap)) return UNETK_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int n = H * W;
  const size_t nb = gc_n_bytes(H, W);
  char* p = (char*)ws;
  int* label = (int*)p;                                   // the layout of unetk_largest_component: label, then size
  int* cnt = (int*)(p + nb);
  int* cid = (int*)(p + 2 * nb);
  uint8_t* mask = (uint8_t*)(p + 3 * nb);
  char* q = p + 3 * nb + ev_align((size_t)n);
  unsigned long long* best = (unsigned long long*)q;      // lc_init's scalars, unused here
  int32_t* info = (int32_t*)(q + 16);
  int* hrow = (int*)(q + 256);
  int* hcol = (int*)(q + 256 + ev_align((size_t)cap * H * 4));
  unsigned long long* peak = (unsigned long long*)(q + 256 + ev_align((size_t)cap * H * 4) + ev_align((size_t)cap * W * 4));
  const int g = ev_grid1(n);
  UNETK_LAUNCH(gc_mask_kernel, dim3(g), dim3(EV_BLOCK), 0, st, acc, n, mask);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(lc_init_kernel, dim3(g), dim3(EV_BLOCK), 0, st, (const uint8_t*)mask, n, label, cnt, best, info);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(lc_merge_kernel, dim3(g), dim3(EV_BLOCK), 0, st, (const uint8_t*)mask, 1, H, W, label);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(lc_flatten_kernel, dim3(g), dim3(EV_BLOCK), 0, st, n, label, cnt);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(gc_enum_kernel, dim3(1), dim3(GC_ENUM), 0, st, n, (const int*)label, (const int*)cnt, cap, cid, table);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(gc_zero_kernel, dim3(min(cap, GC_ZERO_BLOCKS)), dim3(EV_BLOCK), 0, st, (const int32_t*)table, cap, H, W, hrow,
               hcol, peak);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(gc_accum_kernel, dim3(g), dim3(EV_BLOCK), 0, st, n, H, W, (const int*)label, (const int*)cid, guide, cap, hrow,
               hcol, peak);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(gc_final_kernel, dim3((cap + EV_BLOCK - 1) / EV_BLOCK), dim3(EV_BLOCK), 0, st, H, W, cap, (const int*)hrow,
               (const int*)hcol, (const unsigned long long*)peak, table);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

// ---------------------------------------------------------------- component overlaps
static inline bool co_caps_ok(int cap_obj, int cap_pair) {
  return cap_obj > 0 && cap_pair > 0 && cap_obj <= CO_MAX_CAP && cap_pair <= CO_MAX_CAP;
}

// workspace: label of res, label of ref, size of res, size of ref (n int32 each; the two size arrays, read into the object
// rows first, are then the n 64-bit slots of the pair table), lc_init's scalars, the tile sums, the pair list and its sorted copy
extern "C" size_t unetk_component_overlaps_ws_bytes(int D, int H, int W, int cap_obj, int cap_pair) {
  if (ev_dims(D, H, W) != UNETK_OK || !co_caps_ok(cap_obj, cap_pair)) return 0;
  const int64_t n = (int64_t)D * H * W;
  return 4 * ev_align((size_t)n * 4) + 256 + ev_align((size_t)2 * co_tiles(n) * 4) + 2 * ev_align((size_t)cap_pair * 8);
}

extern "C" int unetk_component_overlaps(const uint8_t* res, const uint8_t* ref, int D, int H, int W, int cap_obj, int cap_pair,
                                        int32_t* table, void* ws, size_t ws_bytes, void* stream) {
  const int dims = ev_dims(D, H, W);
  if (dims != UNETK_OK) return dims;
  UNETK_REQUIRE(res && ref && table && ws && unetk_aligned16(ws) && (((uintptr_t)table) & 3u) == 0);
  UNETK_REQUIRE(co_caps_ok(cap_obj, cap_pair));
  if (ws_bytes < unetk_component_overlaps_ws_bytes(D, H, W, cap_obj, cap_pair)) return UNETK_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int n = D * H * W, nt = co_tiles(n);
  const size_t nb = ev_align((size_t)n * 4);
  char* p = (char*)ws;
  int* lres = (int*)p;
  int* lref = (int*)(p + nb);
  int* cres = (int*)(p + 2 * nb);
  int* cref = (int*)(p + 3 * nb);
  unsigned long long* slots = (unsigned long long*)(p + 2 * nb);      // over cres and cref, once the rows hold the sizes
  char* q = p + 4 * nb;
  unsigned long long* best = (unsigned long long*)q;                  // lc_init's scalars, unused here
  int32_t* info = (int32_t*)(q + 16);
  int* tsum = (int*)(q + 256);
  unsigned long long* list = (unsigned long long*)(q + 256 + ev_align((size_t)2 * nt * 4));
  unsigned long long* sorted = list + ev_align((size_t)cap_pair * 8) / 8;
  const int64_t words = 4 + 4 * (int64_t)cap_obj + 3 * (int64_t)cap_pair;
  const int g = ev_grid1(n);
  UNETK_LAUNCH(sh_zero_kernel, dim3(ev_blocks(words)), dim3(EV_BLOCK), 0, st, table, words);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(lc_init_kernel, dim3(g), dim3(EV_BLOCK), 0, st, res, n, lres, cres, best, info);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(lc_merge_kernel, dim3(g), dim3(EV_BLOCK), 0, st, res, D, H, W, lres);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(lc_flatten_kernel, dim3(g), dim3(EV_BLOCK), 0, st, n, lres, cres);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(lc_init_kernel, dim3(g), dim3(EV_BLOCK), 0, st, ref, n, lref, cref, best, info);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(lc_merge_kernel, dim3(g), dim3(EV_BLOCK), 0, st, ref, D, H, W, lref);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(lc_flatten_kernel, dim3(g), dim3(EV_BLOCK), 0, st, n, lref, cref);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(co_tile_roots_kernel, dim3(nt, 2), dim3(EV_BLOCK), 0, st, n, (const int*)lres, (const int*)lref, nt, tsum);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(co_scan_kernel, dim3(2), dim3(CO_SCAN), 0, st, nt, tsum, cap_obj, table);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(co_rows_kernel, dim3(nt, 2), dim3(EV_BLOCK), 0, st, n, (const int*)lres, (const int*)lref, (const int*)cres,
               (const int*)cref, nt, (const int*)tsum, cap_obj, table);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(co_fill_kernel, dim3(ev_blocks(n)), dim3(EV_BLOCK), 0, st, slots, (int64_t)n, CO_EMPTY);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(co_insert_kernel, dim3(g), dim3(EV_BLOCK), 0, st, n, (const int*)lres, (const int*)lref, slots);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(co_compact_kernel, dim3(ev_blocks(n)), dim3(EV_BLOCK), 0, st, n, (const unsigned long long*)slots, cap_pair, list,
               table);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(co_rank_kernel, dim3((cap_pair + EV_BLOCK - 1) / EV_BLOCK), dim3(EV_BLOCK), 0, st,
               (const unsigned long long*)list, cap_obj, cap_pair, sorted, table);
  UNETK_LAUNCH_CHECK();
  UNETK_LAUNCH(co_count_kernel, dim3(g), dim3(EV_BLOCK), 0, st, n, (const int*)lres, (const int*)lref,
               (const unsigned long long*)sorted, cap_obj, cap_pair, table);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}
