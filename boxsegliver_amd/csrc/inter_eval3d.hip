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
// The kernels' bodies from pick to far are inter_click.h's, shared with inter_eval.hip; here: the resident prediction, the
// sweep along z, the workspace that reuses the size words, the finish kernel.
#include "inter_click.h"     // IC_BLOCK, IC_PER_THREAD, IC3_MAX_DEPTH (the key's bit budget)

namespace {

constexpr int IC3_TW = UNETK_INTER3D_TAB_COLS;
using Ic3 = IcDim<3>;
using Sl = IcSlots<3>;                   // header [HD_N]: HD_SUM + 0 / 1 / 2 = the z / y / x sums; info [IF_N]: IF_C + 0 / 1 / 2 = the candidate

inline size_t ic3_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline int64_t ic3_vox(const unetk_inter_click3d_desc* d) { return (int64_t)d->depth * d->src_h * d->src_w; }

struct Ic3Ws {
  unsigned long long* hdr;   // [Sl::HD_N]
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
  o += ic3_align(Sl::HD_N * 8);
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

// ------------------------------------------------------------------------------------------------ err, counts, label init
__global__ __launch_bounds__(IC_BLOCK) void ic3_err_kernel(unetk_inter_click3d_desc d, int64_t vox, const uint8_t* __restrict__ segs,
                                                           const uint8_t* __restrict__ pred, Ic3Ws w) {
  const int thr = d.obj_label * d.lab_scale;
  const uint8_t* seg = segs + (int64_t)d.case_base * d.src_h * d.src_w;   // the case's slices are contiguous in the store
  IcTally t;
#pragma unroll
  for (int u = 0; u < IC_PER_THREAD; ++u) {
    const int64_t i = ic_strided<3>(u);
    if (i < vox) ic_mark(t, pred ? (pred[i] != 0 ? 1 : 0) : 0, (int)seg[i] >= thr ? 1 : 0, i, w.err, w.label, w.cnt);
  }
  ic_tally(t, w.hdr);
}

// ------------------------------------------------------------------------------------------------ components
__global__ __launch_bounds__(IC_BLOCK) void ic3_merge_kernel(unetk_inter_click3d_desc d, int64_t vox, Ic3Ws w) {
  const int64_t i64 = (int64_t)blockIdx.x * IC_BLOCK + threadIdx.x;
  if (i64 >= vox || !w.err[i64]) return;
  int c[3];
  ic_coords<3>((int)i64, d.src_w, d.src_h * d.src_w, c);
  lc_union_back6(w.err, w.label, (int)i64, c[2], c[1], c[0], d.src_w, d.src_h * d.src_w);
}

__global__ __launch_bounds__(IC_BLOCK) void ic3_flatten_kernel(int64_t vox, Ic3Ws w) {
  lc_flatten_count(w.label, w.cnt, (int64_t)blockIdx.x * IC_BLOCK + threadIdx.x, vox);
}

__global__ __launch_bounds__(IC_BLOCK) void ic3_pick_kernel(int64_t vox, Ic3Ws w) { ic_pick<3>(w.label, w.cnt, vox, w.hdr); }

__global__ __launch_bounds__(IC_BLOCK) void ic3_mean_kernel(unetk_inter_click3d_desc d, int64_t vox, Ic3Ws w) {
  ic_mean<3>(w.label, vox, d.src_w, d.src_h * d.src_w, w.hdr);
}

__global__ void ic3_cand_kernel(unetk_inter_click3d_desc d, Ic3Ws w) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  ic_cand<3>(w.hdr, w.info, w.err, d.src_w, d.src_h * d.src_w);
}

// ------------------------------------------------------------------------------------------------ fallback: distances
// along y: thread per (z, x)
__global__ __launch_bounds__(64) void ic3_cols_kernel(unetk_inter_click3d_desc d, Ic3Ws w) {
  const int z = blockIdx.y, x = blockIdx.x * 64 + threadIdx.x;
  if (w.info[Sl::IF_FALLBACK] == 0 || x >= d.src_w) return;
  const int64_t o = (int64_t)z * d.src_h * d.src_w + x;
  // the sweep's second field (distance to the nearest error voxel) is not used: it lands in `dist`, which the row pass rewrites
  clk_col_sweeps(w.err + o, true, d.src_w, d.src_h, d.src_w, 1, d.dist_cap, w.gf + o, w.dist + o);
}

// along x: block per (z, y), the row in LDS
__global__ __launch_bounds__(IC_BLOCK) void ic3_rows_kernel(unetk_inter_click3d_desc d, Ic3Ws w) {
  __shared__ int16_t buf[2][1][CLK_MAX_EXTENT];
  if (w.info[Sl::IF_FALLBACK] == 0) return;                  // block-uniform
  const int z = blockIdx.y, y = blockIdx.x, cw = d.src_w;
  const int64_t o = ((int64_t)z * d.src_h + y) * cw;
  ic_row_pass(buf, w.gf + o, w.dist + o, cw, d.dist_cap);
}

// along z: thread per (y, x), down and up, in place; the case's first and last slice border on non-error
__global__ __launch_bounds__(IC_BLOCK) void ic3_deep_kernel(unetk_inter_click3d_desc d, Ic3Ws w) {
  const int plane = d.src_h * d.src_w, p = blockIdx.x * IC_BLOCK + threadIdx.x;
  if (w.info[Sl::IF_FALLBACK] == 0 || p >= plane) return;
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

__global__ __launch_bounds__(IC_BLOCK) void ic3_far_kernel(unetk_inter_click3d_desc d, int64_t vox, Ic3Ws w) {
  ic_far<3>(w.label, w.dist, vox, d.src_w, d.src_h * d.src_w, w.info, w.hdr);
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
      int z = f[IF_C], y = f[IF_C + 1], x = f[IF_C + 2];
      const int plane = d.src_h * d.src_w;
      out[4] = f[Sl::IF_AREA];
      out[5] = f[Sl::IF_ROOT];
      out[6] = z;
      out[7] = y;
      out[8] = x;
      if (f[Sl::IF_FALLBACK]) {
        const int i = ic_far_index<Ic3::D2_BITS, Ic3::IDX_BITS>(h[Sl::HD_FAR]);   // the component has a voxel: the key is not zero
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
         ic3_vox(d) < ((int64_t)1 << Ic3::IDX_BITS);   // an int holds a voxel index, and the key its field
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
    const dim3 per_voxel((unsigned)((vox + IC_BLOCK - 1) / IC_BLOCK));
    const dim3 strided((unsigned)((vox + IC_BLOCK * IC_PER_THREAD - 1) / (IC_BLOCK * IC_PER_THREAD)));
    const hipError_t e = hipMemsetAsync(ws, 0, lay.zero, st);
    if (e != hipSuccess) return (int)e;
    UNETK_LAUNCH(ic3_err_kernel, strided, dim3(IC_BLOCK), 0, st, *d, vox, seg_slices, pred, w);
    UNETK_LAUNCH(ic3_merge_kernel, per_voxel, dim3(IC_BLOCK), 0, st, *d, vox, w);
    UNETK_LAUNCH(ic3_flatten_kernel, per_voxel, dim3(IC_BLOCK), 0, st, vox, w);
    UNETK_LAUNCH(ic3_pick_kernel, strided, dim3(IC_BLOCK), 0, st, vox, w);
    UNETK_LAUNCH(ic3_mean_kernel, strided, dim3(IC_BLOCK), 0, st, *d, vox, w);
    UNETK_LAUNCH(ic3_cand_kernel, dim3(1), dim3(64), 0, st, *d, w);
    UNETK_LAUNCH(ic3_cols_kernel, dim3((d->src_w + 63) / 64, d->depth), dim3(64), 0, st, *d, w);
    UNETK_LAUNCH(ic3_rows_kernel, dim3(d->src_h, d->depth), dim3(IC_BLOCK), 0, st, *d, w);
    UNETK_LAUNCH(ic3_deep_kernel, dim3((plane + IC_BLOCK - 1) / IC_BLOCK), dim3(IC_BLOCK), 0, st, *d, w);
    UNETK_LAUNCH(ic3_far_kernel, strided, dim3(IC_BLOCK), 0, st, *d, vox, w);
  }
  UNETK_LAUNCH(ic3_finish_kernel, dim3(1), dim3(64), 0, st, *d, inside ? 1 : 2, seg_slices, prev_z, prev_y, prev_x, w, pts, cnt, table);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}
