// The click step of the 3-D interactive evaluator (entry/main_eval_3d.py): the reference's
// inter_simulation_test (entry/main_eval_3d.py:152-185) for ONE case, on the labels of the resident slice store and the case's
// resident prediction volume.  i = (z * src_h + y) * src_w + x is a voxel's linear index inside the case.
//   ic3_err_kernel     ref = stored label >= obj_label * lab_scale; err = pred xor ref; n_pred, n_ref, n_inter
//   ic3_merge / ic3_flatten   6-connected components of err by the union-find of unionfind.h: every voxel ends at the minimum
//                      linear index of its component, sizes at the roots
//   ic3_pick_kernel    the largest component, the SMALLEST root on ties (np.argmax takes the first maximum; scipy numbers the
//                      components by their first voxel in (z, y, x) order, which is the root)
//   ic3_mean_kernel    coordinate sums of the component;  ic3_cand_kernel: their mean per axis, rounded half to even
//   fallback, only where err is not set at the mean (block-uniform early exits elsewhere): capped city-block distance to
//                      the nearest non-error voxel by three separable min-plus passes -- the column sweeps of lits_clicks.h
//                      along y, its min-plus row pass along x, two sweeps along z -- then the arg-max over the component by
//                      one 64-bit key: distance, then the smaller squared distance to the mean, then the smaller linear index
//   ic3_finish_kernel  the click's kind, the append to the case's lists, the table row
// Integer arithmetic only.  The sums and maxima are integer atomics, which commute exactly: two calls give identical bits.
#include "common.h"
#include "lits_clicks.h"     // CLK_MAX_EXTENT, clk_col_sweeps, clk_row_minplus
#include "unionfind.h"

namespace {

constexpr int IC3_BLOCK = 256;
constexpr int IC3_PER_THREAD = 8;        // voxels a thread of the reducing kernels walks
constexpr int IC3_MAX_DEPTH = 4096;      // the fallback key holds the squared distance to the mean in 25 bits
constexpr int IC3_TW = UNETK_INTER3D_TAB_COLS;
enum { HD_NPRED = 0, HD_NREF, HD_NINTER, HD_NCOMP, HD_BEST, HD_SZ, HD_SY, HD_SX, HD_FAR, HD_N };
enum { IF_CZ = 0, IF_CY, IF_CX, IF_FALLBACK, IF_ROOT, IF_AREA, IF_N = 8 };

inline size_t ic3_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline int64_t ic3_vox(const unetk_inter_click3d_desc* d) { return (int64_t)d->depth * d->src_h * d->src_w; }

struct Ic3Ws {
  unsigned long long* hdr;   // [HD_N]
  int32_t* info;             // [IF_N]
  uint8_t *err, *gf, *dist;  // [vox]; gf and dist live in `cnt`, which is dead once the component is picked
  int *label, *cnt;          // [vox]
};
// byte offsets of the fields above; [0, zero) is cleared before every call
struct Ic3Layout {
  size_t hdr, info, zero, err, label, cnt, total;
};
inline Ic3Layout ic3_layout(const unetk_inter_click3d_desc* d) {
  const size_t vox = (size_t)ic3_vox(d);
  Ic3Layout l;
  size_t o = 0;
  l.hdr = o;
  o += ic3_align(HD_N * 8);
  l.info = o;
  o += ic3_align(IF_N * 4);
  l.zero = o;
  l.err = o;
  o += ic3_align(vox);
  l.label = o;
  o += ic3_align(vox * 4);
  l.cnt = o;
  o += ic3_align(vox * 4);
  l.total = o;
  return l;
}
inline Ic3Ws ic3_carve(const Ic3Layout& l, void* ws, size_t vox) {
  char* p = static_cast<char*>(ws);
  Ic3Ws w;
  w.hdr = reinterpret_cast<unsigned long long*>(p + l.hdr);
  w.info = reinterpret_cast<int32_t*>(p + l.info);
  w.err = reinterpret_cast<uint8_t*>(p + l.err);
  w.label = reinterpret_cast<int*>(p + l.label);
  w.cnt = reinterpret_cast<int*>(p + l.cnt);
  w.gf = reinterpret_cast<uint8_t*>(p + l.cnt);
  w.dist = w.gf + vox;
  return w;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(v, o);
    v = other > v ? other : v;
  }
  return v;
}
__device__ __forceinline__ int ic3_root_of(unsigned long long best) { return (int)(0xffffffffu - (unsigned)(best & 0xffffffffull)); }

// ------------------------------------------------------------------------------------------------ err, counts, label init
__global__ __launch_bounds__(IC3_BLOCK) void ic3_err_kernel(unetk_inter_click3d_desc d, int64_t vox, const uint8_t* __restrict__ segs,
                                                            const uint8_t* __restrict__ pred, Ic3Ws w) {
  const int thr = d.obj_label * d.lab_scale;
  const uint8_t* seg = segs + (int64_t)d.case_base * d.src_h * d.src_w;   // the case's slices are contiguous in the store
  unsigned long long np = 0, nr = 0, ni = 0;
  const int64_t base = (int64_t)blockIdx.x * IC3_BLOCK * IC3_PER_THREAD;
#pragma unroll
  for (int u = 0; u < IC3_PER_THREAD; ++u) {
    const int64_t i = base + u * IC3_BLOCK + threadIdx.x;
    if (i < vox) {
      const int p = pred ? (pred[i] != 0 ? 1 : 0) : 0;
      const int r = (int)seg[i] >= thr ? 1 : 0;
      const int e = p ^ r;
      w.err[i] = (uint8_t)e;
      w.label[i] = e ? (int)i : -1;
      w.cnt[i] = 0;
      np += p;
      nr += r;
      ni += p & r;
    }
  }
  np = wave_sum(np);
  nr = wave_sum(nr);
  ni = wave_sum(ni);
  if ((threadIdx.x & 63) == 0) {
    if (np) atomicAdd(w.hdr + HD_NPRED, np);
    if (nr) atomicAdd(w.hdr + HD_NREF, nr);
    if (ni) atomicAdd(w.hdr + HD_NINTER, ni);
  }
}

// ------------------------------------------------------------------------------------------------ components
__global__ __launch_bounds__(IC3_BLOCK) void ic3_merge_kernel(unetk_inter_click3d_desc d, int64_t vox, Ic3Ws w) {
  const int64_t i64 = (int64_t)blockIdx.x * IC3_BLOCK + threadIdx.x;
  if (i64 >= vox || !w.err[i64]) return;
  const int i = (int)i64, plane = d.src_h * d.src_w;
  const int z = i / plane, r = i - z * plane;
  const int y = r / d.src_w, x = r - y * d.src_w;
  if (x > 0 && w.err[i - 1]) lc_union(w.label, i, i - 1);
  if (y > 0 && w.err[i - d.src_w]) lc_union(w.label, i, i - d.src_w);
  if (z > 0 && w.err[i - plane]) lc_union(w.label, i, i - plane);
}

// every voxel points straight at its root; sizes by integer atomics at the root's slot, one per wave for the lanes that
// share the wave's first root (evalvol.hip's lc_flatten_kernel)
__global__ __launch_bounds__(IC3_BLOCK) void ic3_flatten_kernel(int64_t vox, Ic3Ws w) {
  const int64_t i = (int64_t)blockIdx.x * IC3_BLOCK + threadIdx.x;
  int r = -1;
  if (i < vox) {
    const int l = w.label[i];
    if (l >= 0) {
      r = lc_find(w.label, l);
      w.label[i] = r;
    }
  }
  const int lead = __builtin_amdgcn_readfirstlane(r >= 0 ? r : 0x7fffffff);
  const unsigned long long same = __ballot(r == lead);
  if (r < 0) return;
  if (r != lead)
    atomicAdd(w.cnt + r, 1);
  else if ((int)__lane_id() == __ffsll((long long)same) - 1)
    atomicAdd(w.cnt + r, __popcll(same));
}

// best = max over roots of (size << 32 | ~root): the largest component, the smaller root on ties
__global__ __launch_bounds__(IC3_BLOCK) void ic3_pick_kernel(int64_t vox, Ic3Ws w) {
  unsigned long long key = 0ull, roots = 0ull;
  const int64_t base = (int64_t)blockIdx.x * IC3_BLOCK * IC3_PER_THREAD;
#pragma unroll
  for (int u = 0; u < IC3_PER_THREAD; ++u) {
    const int64_t i = base + u * IC3_BLOCK + threadIdx.x;
    if (i < vox && w.label[i] == (int)i) {
      const unsigned long long k = ((unsigned long long)(unsigned)w.cnt[i] << 32) | (unsigned long long)(0xffffffffu - (unsigned)i);
      key = k > key ? k : key;
      roots += 1;
    }
  }
  key = wave_max(key);
  roots = wave_sum(roots);
  if ((threadIdx.x & 63) == 0 && roots) {
    atomicMax(w.hdr + HD_BEST, key);
    atomicAdd(w.hdr + HD_NCOMP, roots);
  }
}

__global__ __launch_bounds__(IC3_BLOCK) void ic3_mean_kernel(unetk_inter_click3d_desc d, int64_t vox, Ic3Ws w) {
  const unsigned long long best = w.hdr[HD_BEST];
  if (best == 0ull) return;                                  // no error voxel
  const int root = ic3_root_of(best), plane = d.src_h * d.src_w;
  unsigned long long sz = 0, sy = 0, sx = 0;
  const int64_t base = (int64_t)blockIdx.x * IC3_BLOCK * IC3_PER_THREAD;
#pragma unroll
  for (int u = 0; u < IC3_PER_THREAD; ++u) {
    const int64_t i64 = base + u * IC3_BLOCK + threadIdx.x;
    if (i64 < vox && w.label[i64] == root) {
      const int i = (int)i64, z = i / plane, r = i - z * plane, y = r / d.src_w;
      sz += (unsigned long long)z;
      sy += (unsigned long long)y;
      sx += (unsigned long long)(r - y * d.src_w);
    }
  }
  sz = wave_sum(sz);
  sy = wave_sum(sy);
  sx = wave_sum(sx);
  if ((threadIdx.x & 63) == 0) {
    if (sz) atomicAdd(w.hdr + HD_SZ, sz);
    if (sy) atomicAdd(w.hdr + HD_SY, sy);
    if (sx) atomicAdd(w.hdr + HD_SX, sx);
  }
}

// np.mean(...).round(0) of integers: s / a rounded half to even (the q / r rule unetk_lits3d_clicks documents)
__device__ __forceinline__ int ic3_round_div(unsigned long long s, unsigned long long a) {
  const unsigned long long q = s / a, r = s - q * a;
  if (2 * r > a) return (int)q + 1;
  if (2 * r == a) return (int)(q + (q & 1ull));
  return (int)q;
}
__global__ void ic3_cand_kernel(unetk_inter_click3d_desc d, Ic3Ws w) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const unsigned long long best = w.hdr[HD_BEST];
  if (best == 0ull) return;                                  // info stays zero: no fallback
  const unsigned long long area = best >> 32;
  // inside the case: means of its voxels' coordinates
  const int cz = ic3_round_div(w.hdr[HD_SZ], area), cy = ic3_round_div(w.hdr[HD_SY], area), cx = ic3_round_div(w.hdr[HD_SX], area);
  w.info[IF_CZ] = cz;
  w.info[IF_CY] = cy;
  w.info[IF_CX] = cx;
  w.info[IF_ROOT] = ic3_root_of(best);
  w.info[IF_AREA] = (int)area;
  w.info[IF_FALLBACK] = w.err[((int64_t)cz * d.src_h + cy) * d.src_w + cx] ? 0 : 1;
}

// ------------------------------------------------------------------------------------------------ fallback: distances
// along y: thread per (z, x)
__global__ __launch_bounds__(64) void ic3_cols_kernel(unetk_inter_click3d_desc d, Ic3Ws w) {
  const int z = blockIdx.y, x = blockIdx.x * 64 + threadIdx.x;
  if (w.info[IF_FALLBACK] == 0 || x >= d.src_w) return;
  const int64_t o = (int64_t)z * d.src_h * d.src_w + x;
  // the sweep's second field (distance to the nearest error voxel) is not used: it lands in `dist`, which the row pass rewrites
  clk_col_sweeps(w.err + o, true, d.src_w, d.src_h, d.src_w, 1, d.dist_cap, w.gf + o, w.dist + o);
}

// along x: block per (z, y), the row in LDS
__global__ __launch_bounds__(IC3_BLOCK) void ic3_rows_kernel(unetk_inter_click3d_desc d, Ic3Ws w) {
  __shared__ int16_t buf[2][1][CLK_MAX_EXTENT];
  if (w.info[IF_FALLBACK] == 0) return;                      // block-uniform
  const int z = blockIdx.y, y = blockIdx.x, cw = d.src_w;
  const int64_t o = ((int64_t)z * d.src_h + y) * cw;
  const uint8_t* gf = w.gf + o;
  uint8_t* dist = w.dist + o;
  for (int x = threadIdx.x; x < cw; x += IC3_BLOCK) buf[0][0][x] = (int16_t)min((int)gf[x], min(x + 1, cw - x));   // the case's border
  __syncthreads();
  const int cur = clk_row_minplus<1>(buf, cw, d.dist_cap);
  for (int x = threadIdx.x; x < cw; x += IC3_BLOCK) dist[x] = (uint8_t)min((int)buf[cur][0][x], d.dist_cap);
}

// along z: thread per (y, x), down and up, in place; the case's first and last slice border on non-error
__global__ __launch_bounds__(IC3_BLOCK) void ic3_deep_kernel(unetk_inter_click3d_desc d, Ic3Ws w) {
  const int plane = d.src_h * d.src_w, p = blockIdx.x * IC3_BLOCK + threadIdx.x;
  if (w.info[IF_FALLBACK] == 0 || p >= plane) return;
  uint8_t* dist = w.dist + p;
  int v = 0;
  for (int z = 0; z < d.depth; ++z) {
    v = min((int)dist[(int64_t)z * plane], v + 1);
    dist[(int64_t)z * plane] = (uint8_t)v;
  }
  v = 0;
  for (int z = d.depth - 1; z >= 0; --z) {
    v = min((int)dist[(int64_t)z * plane], v + 1);
    dist[(int64_t)z * plane] = (uint8_t)v;
  }
}

// key = distance (8 bits) | 2^25 - 1 - squared distance to the mean (25 bits: < 4095^2 + 2 * 1023^2) | 2^31 - 1 - index (31 bits)
__global__ __launch_bounds__(IC3_BLOCK) void ic3_far_kernel(unetk_inter_click3d_desc d, int64_t vox, Ic3Ws w) {
  if (w.info[IF_FALLBACK] == 0) return;
  const int plane = d.src_h * d.src_w, root = w.info[IF_ROOT], cz = w.info[IF_CZ], cy = w.info[IF_CY], cx = w.info[IF_CX];
  unsigned long long key = 0ull;
  const int64_t base = (int64_t)blockIdx.x * IC3_BLOCK * IC3_PER_THREAD;
#pragma unroll
  for (int u = 0; u < IC3_PER_THREAD; ++u) {
    const int64_t i64 = base + u * IC3_BLOCK + threadIdx.x;
    if (i64 < vox && w.label[i64] == root) {
      const int i = (int)i64, z = i / plane, r = i - z * plane, y = r / d.src_w, x = r - y * d.src_w;
      const unsigned long long d2 = (unsigned long long)((z - cz) * (z - cz) + (y - cy) * (y - cy) + (x - cx) * (x - cx));
      const unsigned long long k = ((unsigned long long)w.dist[i] << 56) | ((0x1ffffffull - d2) << 31) | (unsigned long long)(0x7fffffff - i);
      key = k > key ? k : key;
    }
  }
  key = wave_max(key);
  if ((threadIdx.x & 63) == 0 && key) atomicMax(w.hdr + HD_FAR, key);
}

// ------------------------------------------------------------------------------------------------ click, lists, table
__global__ void ic3_finish_kernel(unetk_inter_click3d_desc d, int state, const uint8_t* __restrict__ segs, int pz, int py, int px,
                                  Ic3Ws w, int32_t* __restrict__ pts, int32_t* __restrict__ cnt, int32_t* __restrict__ table) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int out[IC3_TW];
#pragma unroll
  for (int j = 0; j < IC3_TW; ++j) out[j] = 0;
  out[5] = out[6] = out[7] = out[8] = out[9] = out[10] = out[11] = out[12] = -1;
  out[17] = state;
  if (state == 1) {
    const unsigned long long* h = w.hdr;
    const int32_t* f = w.info;
    out[0] = (int)h[HD_NPRED];
    out[1] = (int)h[HD_NREF];
    out[2] = (int)h[HD_NINTER];
    out[3] = (int)h[HD_NCOMP];
    if (h[HD_BEST] == 0ull) {
      out[15] = 1;                                            // nothing to correct: no click
    } else {
      int z = f[IF_CZ], y = f[IF_CY], x = f[IF_CX];
      const int plane = d.src_h * d.src_w;
      out[4] = f[IF_AREA];
      out[5] = f[IF_ROOT];
      out[6] = z;
      out[7] = y;
      out[8] = x;
      if (f[IF_FALLBACK]) {
        const int i = 0x7fffffff - (int)(h[HD_FAR] & 0x7fffffffull);   // the component has a voxel: the key is not zero
        z = i / plane;
        y = (i - z * plane) / d.src_w;
        x = i - z * plane - y * d.src_w;
        out[13] = 1;
      }
      const int kind = (int)segs[((int64_t)d.case_base + z) * plane + y * d.src_w + x] >= d.obj_label * d.lab_scale ? 0 : 1;
      out[9] = z;
      out[10] = y;
      out[11] = x;
      out[12] = kind;
      out[14] = (z == pz && y == py && x == px) ? 1 : 0;
      int32_t* c = cnt + kind;
      const int have = min(max(*c, 0), d.K);
      if (have < d.K) {
        int32_t* p = pts + ((int64_t)kind * d.K + have) * 3;
        p[0] = z;
        p[1] = y;
        p[2] = x;
        *c = have + 1;
        out[16] = 1;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < IC3_TW; ++j) table[j] = out[j];
}

bool ic3_valid(const unetk_inter_click3d_desc* d) {
  return d && d->depth > 0 && d->n_slices > 0 && d->src_h > 0 && d->src_w > 0 && d->lab_scale > 0 && d->obj_label > 0 &&
         (int64_t)d->lab_scale * d->obj_label < ((int64_t)1 << 31) && d->K >= 1 && d->dist_cap >= 1 && d->dist_cap <= 255;
}
bool ic3_supported(const unetk_inter_click3d_desc* d) {
  return d->src_h <= CLK_MAX_EXTENT && d->src_w <= CLK_MAX_EXTENT && d->K <= UNETK_INTER_MAX_CLICKS && d->depth <= IC3_MAX_DEPTH &&
         ic3_vox(d) < ((int64_t)1 << 31);
}

}  // namespace

extern "C" size_t unetk_inter_click3d_ws_bytes(const unetk_inter_click3d_desc* d) {
  if (!ic3_valid(d) || !ic3_supported(d)) return 0;
  return ic3_layout(d).total;
}

extern "C" int unetk_inter_click3d(const unetk_inter_click3d_desc* d, const uint8_t* seg_slices, const uint8_t* pred, int prev_z,
                                   int prev_y, int prev_x, int32_t* pts, int32_t* cnt, int32_t* table, void* ws, size_t ws_bytes,
                                   void* stream) {
  UNETK_REQUIRE(ic3_valid(d) && seg_slices && pts && cnt && table && ws);
  UNETK_REQUIRE(((((uintptr_t)pts) | ((uintptr_t)cnt) | ((uintptr_t)table)) & 3u) == 0 && unetk_aligned16(ws));
  if (!ic3_supported(d)) return UNETK_E_UNSUPPORTED;
  if (ws_bytes < unetk_inter_click3d_ws_bytes(d)) return UNETK_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t vox = ic3_vox(d);                              // < 2^31
  const Ic3Layout lay = ic3_layout(d);
  const Ic3Ws w = ic3_carve(lay, ws, (size_t)vox);
  // a case that leaves the store: nothing of it is read, the row says so
  const bool inside = d->case_base >= 0 && (int64_t)d->case_base + d->depth <= d->n_slices;
  if (inside) {
    const int plane = d->src_h * d->src_w;                     // <= 2^20
    const dim3 per_voxel((unsigned)((vox + IC3_BLOCK - 1) / IC3_BLOCK));
    const dim3 strided((unsigned)((vox + IC3_BLOCK * IC3_PER_THREAD - 1) / (IC3_BLOCK * IC3_PER_THREAD)));
    const hipError_t e = hipMemsetAsync(ws, 0, lay.zero, st);
    if (e != hipSuccess) return (int)e;
    UNETK_LAUNCH(ic3_err_kernel, strided, dim3(IC3_BLOCK), 0, st, *d, vox, seg_slices, pred, w);
    UNETK_LAUNCH(ic3_merge_kernel, per_voxel, dim3(IC3_BLOCK), 0, st, *d, vox, w);
    UNETK_LAUNCH(ic3_flatten_kernel, per_voxel, dim3(IC3_BLOCK), 0, st, vox, w);
    UNETK_LAUNCH(ic3_pick_kernel, strided, dim3(IC3_BLOCK), 0, st, vox, w);
    UNETK_LAUNCH(ic3_mean_kernel, strided, dim3(IC3_BLOCK), 0, st, *d, vox, w);
    UNETK_LAUNCH(ic3_cand_kernel, dim3(1), dim3(64), 0, st, *d, w);
    UNETK_LAUNCH(ic3_cols_kernel, dim3((d->src_w + 63) / 64, d->depth), dim3(64), 0, st, *d, w);
    UNETK_LAUNCH(ic3_rows_kernel, dim3(d->src_h, d->depth), dim3(IC3_BLOCK), 0, st, *d, w);
    UNETK_LAUNCH(ic3_deep_kernel, dim3((plane + IC3_BLOCK - 1) / IC3_BLOCK), dim3(IC3_BLOCK), 0, st, *d, w);
    UNETK_LAUNCH(ic3_far_kernel, strided, dim3(IC3_BLOCK), 0, st, *d, vox, w);
  }
  UNETK_LAUNCH(ic3_finish_kernel, dim3(1), dim3(64), 0, st, *d, inside ? 1 : 2, seg_slices, prev_z, prev_y, prev_x, w, pts, cnt, table);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}
