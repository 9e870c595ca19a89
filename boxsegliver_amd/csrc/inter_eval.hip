// The click step of the interactive evaluator (entry/main_eval.py): the reference's inter_simulation_test
// (entry/main_eval.py:149-183) for N sessions at once, on the labels of the resident slice store.  Per session:
//   ic_err_kernel     prediction at source resolution (nearest, floor(y * H / src_h)), written into the case's volume;
//                     ref = stored label >= obj_label * lab_scale; err = pred xor ref; n_pred, n_ref, n_inter
//   ic_merge / ic_flatten   4-connected components of err by the union-find of unionfind.h: every pixel ends at the minimum
//                     linear index of its component, sizes at the roots
//   ic_pick_kernel    the largest component, the SMALLEST root on ties (np.argmax takes the first maximum; scipy numbers the
//                     components by their first pixel in row-major order, which is the root)
//   ic_mean_kernel    coordinate sums of the component;  ic_cand_kernel: their mean per axis, rounded half to even
//   fallback, only where err is not set at the mean (block-uniform early exits elsewhere): capped city-block distance to
//                     the nearest non-error pixel (column sweeps of lits_clicks.h, min-plus row pass), then the arg-max over
//                     the component by one 64-bit key: distance, then the smaller squared distance to the mean, then the
//                     smaller linear index
//   ic_finish_kernel  the click's kind, the append to the session's lists, the table row
// Integer arithmetic only.  The sums and maxima are integer atomics, which commute exactly: two calls give identical bits.
// The kernels' bodies from pick to far are inter_click.h's, shared with inter_eval3d.hip; here: which sessions run, the
// resize of the prediction, the addresses of a session's planes, the finish kernel.
#include "inter_click.h"

namespace {

constexpr int IC_CAP = 255;              // the distance cap: a byte (clk_col_sweeps wants <= 255, the key holds 8 bits)
constexpr int IC_TW = UNETK_INTER_TAB_COLS, IC_RW = UNETK_INTER_ROW_COLS;
static_assert(IC_CAP <= 255, "a distance is a byte");
using Ic = IcDim<2>;
using Sl = IcSlots<2>;                   // header [HD_N]: HD_SUM + 0 / 1 = the y / x sums; info [IF_N]: IF_C + 0 / 1 = the candidate's y / x

inline size_t ic_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline int ic_blocks(int plane) { return (plane + IC_BLOCK * IC_PER_THREAD - 1) / (IC_BLOCK * IC_PER_THREAD); }

struct IcWs {
  unsigned long long* hdr;   // [N][Sl::HD_N]
  int32_t* info;             // [N][IF_N]
  uint8_t *err, *gf, *dist;  // [N][plane]
  int *label, *cnt;          // [N][plane]
};
// byte offsets of the fields above; [0, zero) is cleared before every call
struct IcLayout {
  size_t hdr, info, zero, err, gf, dist, label, cnt, total;
};
inline IcLayout ic_layout(const unetk_inter_click_desc* d) {
  const size_t plane = (size_t)d->src_h * d->src_w, n = (size_t)d->N;
  IcLayout l;
  size_t o = 0;
  l.hdr = o;
  o += ic_align(n * Sl::HD_N * 8);
  l.info = o;
  o += ic_align(n * IF_N * 4);
  l.zero = o;
  l.err = o;
  o += ic_align(n * plane);
  l.gf = o;
  o += ic_align(n * plane);
  l.dist = o;
  o += ic_align(n * plane);
  l.label = o;
  o += ic_align(n * plane * 4);
  l.cnt = o;
  o += ic_align(n * plane * 4);
  l.total = o;
  return l;
}
inline IcWs ic_carve(const IcLayout& l, void* ws) {
  char* p = static_cast<char*>(ws);
  IcWs w;
  w.hdr = reinterpret_cast<unsigned long long*>(p + l.hdr);
  w.info = reinterpret_cast<int32_t*>(p + l.info);
  w.err = reinterpret_cast<uint8_t*>(p + l.err);
  w.gf = reinterpret_cast<uint8_t*>(p + l.gf);
  w.dist = reinterpret_cast<uint8_t*>(p + l.dist);
  w.label = reinterpret_cast<int*>(p + l.label);
  w.cnt = reinterpret_cast<int*>(p + l.cnt);
  return w;
}

// row state: 1 = runs, 0 = inactive, 2 = a slice index outside the store or the volume (nothing is read or written for it)
__device__ __forceinline__ int ic_state(const unetk_inter_click_desc& d, const int32_t* __restrict__ rows, int n, bool has_vol) {
  const int32_t* r = rows + (int64_t)n * IC_RW;
  if (r[1] == 0) return 0;
  const int64_t s = r[0], v = s - d.vol_base;
  if (s < 0 || s >= d.n_slices || (has_vol && (v < 0 || v >= d.vol_depth))) return 2;
  return 1;
}

// ------------------------------------------------------------------------------------------------ err, counts, label init
__global__ __launch_bounds__(IC_BLOCK) void ic_err_kernel(unetk_inter_click_desc d, const uint8_t* __restrict__ segs,
                                                          const int32_t* __restrict__ rows, const uint8_t* __restrict__ pred,
                                                          uint8_t* __restrict__ vol, IcWs w) {
  const int n = blockIdx.y;
  if (ic_state(d, rows, n, vol != nullptr) != 1) return;     // block-uniform
  const int plane = d.src_h * d.src_w, thr = d.obj_label * d.lab_scale;
  const int64_t sl = rows[(int64_t)n * IC_RW];
  const uint8_t* seg = segs + sl * plane;
  const uint8_t* pr = pred ? pred + (int64_t)n * d.H * d.W : nullptr;
  uint8_t* vo = vol ? vol + (sl - d.vol_base) * plane : nullptr;
  uint8_t* err = w.err + (int64_t)n * plane;
  int* label = w.label + (int64_t)n * plane;
  int* cnt = w.cnt + (int64_t)n * plane;
  IcTally t;
#pragma unroll
  for (int u = 0; u < IC_PER_THREAD; ++u) {
    const int i = ic_strided<2>(u);
    if (i < plane) {
      const int y = i / d.src_w, x = i - y * d.src_w;
      const int p = pr ? (pr[(y * d.H / d.src_h) * d.W + x * d.W / d.src_w] != 0 ? 1 : 0) : 0;   // y * H < 2^31: ic_supported
      const int r = (int)seg[i] >= thr ? 1 : 0;
      if (vo) vo[i] = (uint8_t)p;
      ic_mark(t, p, r, i, err, label, cnt);
    }
  }
  ic_tally(t, w.hdr + (int64_t)n * Sl::HD_N);
}

// ------------------------------------------------------------------------------------------------ components
__global__ __launch_bounds__(IC_BLOCK) void ic_merge_kernel(unetk_inter_click_desc d, const int32_t* __restrict__ rows,
                                                            bool has_vol, IcWs w) {
  const int n = blockIdx.y;
  if (ic_state(d, rows, n, has_vol) != 1) return;
  const int plane = d.src_h * d.src_w, i = blockIdx.x * IC_BLOCK + threadIdx.x;
  const uint8_t* err = w.err + (int64_t)n * plane;
  int* label = w.label + (int64_t)n * plane;
  if (i >= plane || !err[i]) return;
  const int y = i / d.src_w;
  lc_union_back6(err, label, i, i - y * d.src_w, y, 0, d.src_w, plane);
}

__global__ __launch_bounds__(IC_BLOCK) void ic_flatten_kernel(unetk_inter_click_desc d, const int32_t* __restrict__ rows,
                                                              bool has_vol, IcWs w) {
  const int n = blockIdx.y;
  if (ic_state(d, rows, n, has_vol) != 1) return;
  const int plane = d.src_h * d.src_w;
  lc_flatten_count(w.label + (int64_t)n * plane, w.cnt + (int64_t)n * plane, (int)(blockIdx.x * IC_BLOCK + threadIdx.x), plane);
}

__global__ __launch_bounds__(IC_BLOCK) void ic_pick_kernel(unetk_inter_click_desc d, const int32_t* __restrict__ rows,
                                                           bool has_vol, IcWs w) {
  const int n = blockIdx.y;
  if (ic_state(d, rows, n, has_vol) != 1) return;
  const int plane = d.src_h * d.src_w;
  ic_pick<2>(w.label + (int64_t)n * plane, w.cnt + (int64_t)n * plane, plane, w.hdr + (int64_t)n * Sl::HD_N);
}

__global__ __launch_bounds__(IC_BLOCK) void ic_mean_kernel(unetk_inter_click_desc d, const int32_t* __restrict__ rows,
                                                           bool has_vol, IcWs w) {
  const int n = blockIdx.y;
  if (ic_state(d, rows, n, has_vol) != 1) return;
  const int plane = d.src_h * d.src_w;
  ic_mean<2>(w.label + (int64_t)n * plane, plane, d.src_w, plane, w.hdr + (int64_t)n * Sl::HD_N);
}

__global__ void ic_cand_kernel(unetk_inter_click_desc d, const int32_t* __restrict__ rows, bool has_vol, IcWs w) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= d.N || ic_state(d, rows, n, has_vol) != 1) return;
  const int plane = d.src_h * d.src_w;
  ic_cand<2>(w.hdr + (int64_t)n * Sl::HD_N, w.info + (int64_t)n * IF_N, w.err + (int64_t)n * plane, d.src_w, plane);
}

// ------------------------------------------------------------------------------------------------ fallback: distances
__global__ __launch_bounds__(64) void ic_cols_kernel(unetk_inter_click_desc d, IcWs w) {
  const int n = blockIdx.y, x = blockIdx.x * 64 + threadIdx.x;
  if (w.info[(int64_t)n * IF_N + Sl::IF_FALLBACK] == 0 || x >= d.src_w) return;   // zero for rows that do not run
  const int64_t plane = (int64_t)d.src_h * d.src_w;
  // the sweep's second field (distance to the nearest error pixel) is not used: it lands in `dist`, which the row pass rewrites
  clk_col_sweeps(w.err + n * plane + x, true, d.src_w, d.src_h, d.src_w, 1, IC_CAP, w.gf + n * plane + x, w.dist + n * plane + x);
}

__global__ __launch_bounds__(IC_BLOCK) void ic_rows_kernel(unetk_inter_click_desc d, IcWs w) {
  __shared__ int16_t buf[2][1][CLK_MAX_EXTENT];
  const int n = blockIdx.y, y = blockIdx.x;
  if (w.info[(int64_t)n * IF_N + Sl::IF_FALLBACK] == 0) return;  // block-uniform
  const int64_t o = n * ((int64_t)d.src_h * d.src_w) + (int64_t)y * d.src_w;
  ic_row_pass(buf, w.gf + o, w.dist + o, d.src_w, IC_CAP);
}

__global__ __launch_bounds__(IC_BLOCK) void ic_far_kernel(unetk_inter_click_desc d, IcWs w) {
  const int n = blockIdx.y, plane = d.src_h * d.src_w;
  ic_far<2>(w.label + (int64_t)n * plane, w.dist + (int64_t)n * plane, plane, d.src_w, plane, w.info + (int64_t)n * IF_N,
            w.hdr + (int64_t)n * Sl::HD_N);
}

// ------------------------------------------------------------------------------------------------ click, lists, table
__global__ void ic_finish_kernel(unetk_inter_click_desc d, const uint8_t* __restrict__ segs, const int32_t* __restrict__ rows,
                                 bool has_vol, IcWs w, int32_t* __restrict__ pts, int32_t* __restrict__ cnt,
                                 int32_t* __restrict__ table) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= d.N) return;
  int32_t* t = table + (int64_t)n * IC_TW;
  const int state = ic_state(d, rows, n, has_vol);
  int out[IC_TW];
#pragma unroll
  for (int j = 0; j < IC_TW; ++j) out[j] = 0;
  out[8] = out[9] = out[10] = -1;
  out[15] = state;
  if (state == 1) {
    const unsigned long long* h = w.hdr + (int64_t)n * Sl::HD_N;
    const int32_t* f = w.info + (int64_t)n * IF_N;
    const int32_t* r = rows + (int64_t)n * IC_RW;
    out[0] = (int)h[HD_NPRED];
    out[1] = (int)h[HD_NREF];
    out[2] = (int)h[HD_NINTER];
    out[3] = (int)h[HD_NCOMP];
    if (h[HD_BEST] == 0ull) {
      out[5] = out[6] = out[7] = -1;
      out[13] = 1;                                            // nothing to correct: no click
    } else {
      int y = f[IF_C], x = f[IF_C + 1];
      out[4] = f[Sl::IF_AREA];
      out[5] = f[Sl::IF_ROOT];
      out[6] = y;
      out[7] = x;
      if (f[Sl::IF_FALLBACK]) {
        const int i = ic_far_index<Ic::D2_BITS, Ic::IDX_BITS>(h[Sl::HD_FAR]);   // the component has a pixel: the key is not zero
        y = i / d.src_w;
        x = i - y * d.src_w;
        out[11] = 1;
      }
      const int plane = d.src_h * d.src_w;
      const int kind = (int)segs[(int64_t)r[0] * plane + y * d.src_w + x] >= d.obj_label * d.lab_scale ? 0 : 1;
      out[8] = y;
      out[9] = x;
      out[10] = kind;
      out[12] = (y == r[2] && x == r[3]) ? 1 : 0;
      int32_t* c = cnt + (int64_t)n * 2 + kind;
      const int have = min(max(*c, 0), d.K);
      if (have < d.K) {
        int32_t* p = pts + (((int64_t)n * 2 + kind) * d.K + have) * 2;
        p[0] = y;
        p[1] = x;
        *c = have + 1;
        out[14] = 1;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < IC_TW; ++j) t[j] = out[j];
}

bool ic_valid(const unetk_inter_click_desc* d) {
  return d && d->N > 0 && d->N <= 65535 && d->H > 0 && d->W > 0 && d->n_slices > 0 && d->src_h > 0 && d->src_w > 0 &&
         d->lab_scale > 0 && d->obj_label > 0 && (int64_t)d->lab_scale * d->obj_label < ((int64_t)1 << 31) && d->K >= 1 &&
         d->vol_base >= 0 && d->vol_depth >= 0;
}
bool ic_supported(const unetk_inter_click_desc* d) {
  return d->src_h <= CLK_MAX_EXTENT && d->src_w <= CLK_MAX_EXTENT && d->K <= UNETK_INTER_MAX_CLICKS &&
         (int64_t)d->H * d->W < ((int64_t)1 << 31) / CLK_MAX_EXTENT;     // y * H and the prediction's index stay in an int
}

}  // namespace

extern "C" size_t unetk_inter_click_ws_bytes(const unetk_inter_click_desc* d) {
  if (!ic_valid(d) || !ic_supported(d)) return 0;
  return ic_layout(d).total;
}

extern "C" int unetk_inter_click(const unetk_inter_click_desc* d, const uint8_t* seg_slices, const int32_t* rows,
                                 const uint8_t* pred, uint8_t* vol, int32_t* pts, int32_t* cnt, int32_t* table, void* ws,
                                 size_t ws_bytes, void* stream) {
  UNETK_REQUIRE(ic_valid(d) && seg_slices && rows && pts && cnt && table && ws);
  UNETK_REQUIRE(((((uintptr_t)rows) | ((uintptr_t)pts) | ((uintptr_t)cnt) | ((uintptr_t)table)) & 3u) == 0 && unetk_aligned16(ws));
  if (!ic_supported(d)) return UNETK_E_UNSUPPORTED;
  if (ws_bytes < unetk_inter_click_ws_bytes(d)) return UNETK_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const IcLayout lay = ic_layout(d);
  const IcWs w = ic_carve(lay, ws);
  const int plane = d->src_h * d->src_w;                       // <= 2^20
  const bool has_vol = vol != nullptr;
  const dim3 per_pixel((plane + IC_BLOCK - 1) / IC_BLOCK, d->N), strided(ic_blocks(plane), d->N), per_row((d->N + 63) / 64);
  const hipError_t e = hipMemsetAsync(ws, 0, lay.zero, st);
  if (e != hipSuccess) return (int)e;
  UNETK_LAUNCH(ic_err_kernel, strided, dim3(IC_BLOCK), 0, st, *d, seg_slices, rows, pred, vol, w);
  UNETK_LAUNCH(ic_merge_kernel, per_pixel, dim3(IC_BLOCK), 0, st, *d, rows, has_vol, w);
  UNETK_LAUNCH(ic_flatten_kernel, per_pixel, dim3(IC_BLOCK), 0, st, *d, rows, has_vol, w);
  UNETK_LAUNCH(ic_pick_kernel, strided, dim3(IC_BLOCK), 0, st, *d, rows, has_vol, w);
  UNETK_LAUNCH(ic_mean_kernel, strided, dim3(IC_BLOCK), 0, st, *d, rows, has_vol, w);
  UNETK_LAUNCH(ic_cand_kernel, per_row, dim3(64), 0, st, *d, rows, has_vol, w);
  UNETK_LAUNCH(ic_cols_kernel, dim3((d->src_w + 63) / 64, d->N), dim3(64), 0, st, *d, w);
  UNETK_LAUNCH(ic_rows_kernel, dim3(d->src_h, d->N), dim3(IC_BLOCK), 0, st, *d, w);
  UNETK_LAUNCH(ic_far_kernel, strided, dim3(IC_BLOCK), 0, st, *d, w);
  UNETK_LAUNCH(ic_finish_kernel, per_row, dim3(64), 0, st, *d, seg_slices, rows, has_vol, w, pts, cnt, table);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}
