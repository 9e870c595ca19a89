// slim.conv3d (NetworksV2/UNet3D.py:153,165) with kernels (1,3,3) / (3,3,3), strides 1 / (1,2,2) / (2,2,2),
// TF `SAME` padding (asymmetric for even sizes at stride 2: 0 before, 1 after -- SURVEY.md B2), no bias.
//
// Composition over the 2-D fp32-MFMA kernels instead of a separate 3-D kernel family:
//   * a (kd,3,3) conv is the sum over depth taps dt of (1,3,3) convs on depth-shifted planes; each tap is ONE
//     launch of conv3x3_igemm over the (n, d_out) planes, addressed in place through ImgAddr (depth slices /
//     depth-strided views, no copies), accumulating into the output (epilogue y += acc); the tap that covers
//     every output plane runs last and produces the norm statistics.  Depth stride 2 is just a plane stride.
//   * H/W stride 2 (10.7 % of UNet3D's FLOPs): forward = the igemm kernel's native stride-2 tile (conv_igemm.hip,
//     S = 2) when Cin % 16 == 0 and Cout % 64 == 0, else stride-1 conv into a scratch tensor + subsample (which also
//     emits the statistic partials); input gradient = four output-parity classes contracted from the UNDILATED dy
//     (conv_igemm_lin.hip, GEN variant) when Cin % 64 == 0, else dilate dy + the stride-1 kernel; filter gradient =
//     dilate dy (zero insertion) + the stride-1 kernel, dW = wgrad_s1(x, dilate(dy)) exactly, at 4x MFMA work (a
//     parity-plane variant was measured and dropped: it stages the same bytes, which is what bounds that kernel).
#include "common.h"

namespace {

struct Geo3 {
  int Do, Ho, Wo;       // output extents
  int pb_d;             // SAME pad-before in depth
  int off_h, off_w;     // position of output (ho, wo) in the stride-1 result: 2*ho + off  (stride 2 only)
};

inline int same_pb(int in, int k, int s) {
  const int out = (in + s - 1) / s;
  int total = (out - 1) * s + k - in;
  if (total < 0) total = 0;
  return total / 2;
}

Geo3 geo3(const unetk_conv3d_desc* d) {
  Geo3 g;
  g.Do = (d->D + d->sd - 1) / d->sd;
  g.Ho = (d->H + d->shw - 1) / d->shw;
  g.Wo = (d->W + d->shw - 1) / d->shw;
  g.pb_d = same_pb(d->D, d->kd, d->sd);
  // stride-1 conv pads 1 before; stride-2 SAME pads pb before => y_s2[o] = y_s1[2*o + 1 - pb]
  g.off_h = 1 - same_pb(d->H, 3, 2);
  g.off_w = 1 - same_pb(d->W, 3, 2);
  return g;
}

// valid output-plane range of depth tap dt: 0 <= do*sd - pb + dt < D
inline void tap_range(const unetk_conv3d_desc* d, const Geo3& g, int dt, int* lo, int* hi) {
  int l = g.pb_d - dt;
  l = l <= 0 ? 0 : (l + d->sd - 1) / d->sd;
  int h = (d->D - 1 + g.pb_d - dt);
  h = h < 0 ? -1 : h / d->sd;
  if (h > g.Do - 1) h = g.Do - 1;
  *lo = l;
  *hi = h;
}

bool desc_ok(const unetk_conv3d_desc* d) {
  return d && d->N > 0 && d->D > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0 &&
         (d->kd == 1 || d->kd == 3) && (d->sd == 1 || d->sd == 2) && (d->shw == 1 || d->shw == 2) &&
         !(d->kd == 1 && d->sd != 1) && d->x_stride >= d->Cin && d->y_stride >= d->Cout;
}

// blocks of 256 threads for a grid-stride loop over `work` elements
inline int ew_grid(int64_t work) { return work > (int64_t)8192 * 256 ? 8192 : (int)((work + 255) / 256); }

// zero the C channels of npix pixels at pixel stride `stride`: an output that is a channel slice of a concat buffer must leave
// the channels beside it alone (a dense output is one memset)
__global__ __launch_bounds__(256) void zero_slice_kernel(float* __restrict__ p, int64_t npix, int C, int stride) {
  const int64_t total = npix * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t px = i / C;
    p[px * stride + (i - px * C)] = 0.f;
  }
}

int zero_pixels(float* p, int64_t npix, int C, int stride, hipStream_t st) {
  if (stride == C) {
    const hipError_t e = hipMemsetAsync(p, 0, (size_t)npix * C * sizeof(float), st);
    return e == hipSuccess ? UNETK_OK : (int)e;
  }
  UNETK_LAUNCH(zero_slice_kernel, dim3(ew_grid(npix * C)), dim3(256), 0, st, p, npix, C, stride);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

// y[n, do, ho, wo, :] = t[n, do, 2ho+off_h, 2wo+off_w, :]; statistic partials per block, blocks grouped per sample
__global__ __launch_bounds__(256) void subsample2_stats_kernel(const float* __restrict__ t, float* __restrict__ y,
                                                               float* __restrict__ stat, int planes_per_sample, int H,
                                                               int W, int Ho, int Wo, int C, int ys, int off_h,
                                                               int off_w, int cq_n, int rpi, int bps, int stat_rows) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [2][rpi][C]
  const int cq = threadIdx.x % cq_n, rl = threadIdx.x / cq_n;
  const int n = blockIdx.x / bps, blk = blockIdx.x % bps;
  const int64_t P = (int64_t)planes_per_sample * Ho * Wo;       // output pixels of this sample
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f), sq = s;
  if (rl < rpi) {
    for (int64_t pix = (int64_t)blk * rpi + rl; pix < P; pix += (int64_t)bps * rpi) {
      const int wo = (int)(pix % Wo);
      const int64_t r = pix / Wo;
      const int ho = (int)(r % Ho);
      const int64_t plane = (int64_t)n * planes_per_sample + r / Ho;
      const float4 v = ldg4(t + ((plane * H + 2 * ho + off_h) * W + 2 * wo + off_w) * C + cq * 4);
      stg4(y + ((int64_t)n * P + pix) * ys + cq * 4, v);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      sq.x += v.x * v.x; sq.y += v.y * v.y; sq.z += v.z * v.z; sq.w += v.w * v.w;
    }
    if (stat != nullptr) {
      stg4(&smem[(0 * rpi + rl) * C + cq * 4], s);
      stg4(&smem[(1 * rpi + rl) * C + cq * 4], sq);
    }
  }
  if (stat == nullptr) return;
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += 256) {
    const int k = i / C, c = i - k * C;
    float v = 0.f;
    for (int j = 0; j < rpi; ++j) v += smem[(k * rpi + j) * C + c];
    stat[((int64_t)k * stat_rows + blockIdx.x) * C + c] = v;
  }
}

// z (pre-zeroed) [planes, H, W, C]: z[p, 2ho+off_h, 2wo+off_w, :] = dy[p, ho, wo, :]
__global__ __launch_bounds__(256) void dilate2_kernel(const float* __restrict__ dy, int dys, float* __restrict__ z,
                                                      int64_t npix_out, int H, int W, int Ho, int Wo, int C, int off_h,
                                                      int off_w) {
  const int cq_n = C >> 2;
  const int64_t total = npix_out * cq_n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int cq = (int)(i % cq_n);
    int64_t r = i / cq_n;
    const int wo = (int)(r % Wo); r /= Wo;
    const int ho = (int)(r % Ho);
    const int64_t plane = r / Ho;
    const float4 v = ldg4(dy + ((plane * Ho + ho) * Wo + wo) * dys + cq * 4);
    stg4(z + ((plane * H + 2 * ho + off_h) * W + 2 * wo + off_w) * C + cq * 4, v);
  }
}

// space-to-depth (round 5): xs[po][ho][wo][cls * C + c] = x[po * sd + cd][2 ho + ph][2 wo + pw][c], cls = (cd * 2 + ph) * 2 + pw
// (cd only with depth stride 2): the parity classes of a strided conv's input side by side on the channel axis, so that the
// conv is a stride-1 contraction over xs with tap subsets (conv_igemm_lin.hip GRP)
__global__ __launch_bounds__(256) void s2d_kernel(const float* __restrict__ x, int xs_in, float* __restrict__ out, int64_t npix_out,
                                                  int Do, int D, int H, int W, int Ho, int Wo, int C, int sd) {
  const int cq_n = C >> 2, ncls = sd == 2 ? 8 : 4;
  const int64_t total = npix_out * ncls * cq_n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int cq = (int)(i % cq_n);
    int64_t r = i / cq_n;
    const int cls = (int)(r % ncls); r /= ncls;
    const int wo = (int)(r % Wo); r /= Wo;
    const int ho = (int)(r % Ho); r /= Ho;
    const int po = (int)(r % Do);
    const int64_t n = r / Do;
    const int cd = cls >> 2, ph = (cls >> 1) & 1, pw = cls & 1;
    const int64_t plane = n * D + (int64_t)po * sd + cd;
    const float4 v = ldg4(x + ((plane * H + 2 * ho + ph) * W + 2 * wo + pw) * xs_in + cq * 4);
    stg4(out + ((((n * Do + po) * Ho + ho) * Wo + wo) * ncls + cls) * (int64_t)C + cq * 4, v);
  }
}

inline ImgAddr planes(int HW_floats, int group, int step, int planes_total) {
  ImgAddr a;
  a.img_stride = (int64_t)step * HW_floats;
  a.group_stride = (int64_t)planes_total * HW_floats;
  a.group = group;
  return a;
}

const int SUB_BPS = 64;   // subsample blocks per sample

// The plan of the 2-D launch over a 3-D layer's planes: `np` images of H x W in samples of spg planes; klive = live channels of
// the contraction axis, kd / ng = fused depth taps / tap groups (they size the stream-K cut).
ConvPlan plane_plan(int np, int H, int W, int Cin, int Cout, int spg, int klive = 0, int kd = 0, int ng = 0, int stride = 1,
                    int bf16 = 0) {
  ConvShape s{};
  s.N = np; s.H = H; s.W = W; s.Cin = Cin; s.Cout = Cout; s.xs = Cin; s.ys = Cout; s.spg = spg;
  s.klive = klive; s.kd = kd; s.ng = ng; s.stride = stride; s.bf16 = bf16;
  return unetk_conv_plan(s);
}
bool is_lin(const ConvPlan& pl) { return pl.family == CONV_LIN || pl.family == CONV_LIN_SK; }

// The plane-launch fields of ConvParams: np planes of H x W in samples of spg planes, x -> y at pixel strides xs / ys
ConvParams plane_params(const float* x, const float* wp, float* y, int np, int H, int W, int Cin, int Cout, int xs, int ys,
                        const ImgAddr& xa, const ImgAddr& ya, int spg) {
  ConvParams p{};
  p.x = x; p.wp = wp; p.y = y;
  p.N = np; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.xs = xs; p.ys = ys;
  p.xa = xa; p.ya = ya; p.spg = spg;
  return p;
}

// UNETK_KSKIP (measurement; read once): bit 0 = skip the dead 16-channel chunks of a channel-padded contraction axis
// (unetk_conv3d_desc.cin_live8 / cout_live8), bit 1 = half the MFMAs on a chunk whose upper 8 channels are padding.  Default 3.
int kskip() { static const int v = unetk_env_int("UNETK_KSKIP", 3); return v; }
int live_k(const uint32_t live8[2], int K) { return (kskip() & 1) ? 16 * unetk_live_chunks(live8, K) : K; }
void set_live(ConvParams& p, const uint32_t live8[2], int K) {
  if (kskip() & 1) unetk_set_klive(p, live8, K, (kskip() & 2) != 0);
}

// The filter-gradient launches of a layer, decided once: the workspace queries size for exactly these (wg_runs_bytes) and the
// entry points launch them (run_wgrad).  Route: stride-2 tiles straight from dy when that kernel takes the channels -- else dy is
// zero-dilated into the first zf floats of the workspace and the stride-1 kernels run on it, dW = wgrad_s1(x, dilate(dy)); all
// three depth taps fused into ONE launch (WgParams::kd) when the plan of that launch takes them -- a third of the splits fills
// the chip, so every block walks three times the tiles and the slab round trip shrinks accordingly -- else one launch per depth
// tap over the output planes lo .. hi the tap reaches.  The split count is not monotone in the planes (unetk_split), so a
// tap's launch is planned at its own plane count.
struct WgRun {
  WgShape s;
  int dt, lo, hi;        // dt < 0: every depth tap in this one launch; hi < lo: the tap reaches no plane (its gradient is zero)
};
struct WgRuns {
  int n;
  WgRun run[3];
  bool native;           // stride-2 tiles of OUTPUT pixels: tap (kh, kw) of output (oh, ow) reads input (2 oh - pb + kh, 2 ow - pb + kw)
  size_t zf;             // floats of the dilated dy in front of the filter gradient's workspace
};
WgRuns wg_runs(const unetk_conv3d_desc* d, const Geo3& g, int prec) {
  WgRuns r{};
  WgShape s{d->N * g.Do, d->H, d->W, d->Cin, d->Cout, prec, 1, 1, 1};
  if (d->shw == 2) {
    WgShape s2 = s;
    s2.H = g.Ho; s2.W = g.Wo; s2.stride = 2;
    r.native = unetk_wgrad_plan(s2).rc == UNETK_OK;
    if (r.native) s = s2;
    else r.zf = ((size_t)d->N * g.Do * d->H * d->W * d->Cout + 63) & ~(size_t)63;
  }
  WgShape sf = s;
  sf.kd = 3;
  if (d->kd == 3 && (r.native || d->shw == 1) && unetk_wgrad_plan(sf).rc == UNETK_OK) {
    r.run[r.n++] = WgRun{sf, -1, 0, g.Do - 1};
    return r;
  }
  for (int dt = 0; dt < d->kd; ++dt) {
    WgRun& t = r.run[r.n++];
    t.s = s; t.dt = dt;
    tap_range(d, g, dt, &t.lo, &t.hi);
    t.s.N = d->N * (t.hi - t.lo + 1);
  }
  return r;
}
size_t wg_runs_bytes(const WgRuns& r) {
  size_t bytes = 0;
  for (int i = 0; i < r.n; ++i) {
    if (r.run[i].hi < r.run[i].lo) continue;
    const WgPlan pl = unetk_wgrad_plan(r.run[i].s);
    if (pl.rc == UNETK_OK && pl.ws_bytes > bytes) bytes = pl.ws_bytes;
  }
  return bytes ? r.zf * sizeof(float) + bytes : 0;
}

// ---- one decision per 3-D conv layer, as ConvPlan / WgPlan (common.h) and DeconvPlan (deconv.hip).  conv3d_plan (pure host
// arithmetic, no HIP calls) derives from the descriptor and the precision the route of each op, the rows of the launch that
// writes the statistics, the workspace and every refusal the descriptor decides; the queries return its fields and the entry
// points launch what it says, so the five cannot disagree.
enum FwdRoute {
  FWD_TAPS,              // one stride-1 launch per depth tap, accumulating when kd == 3
  FWD_FUSED_LIN,         // small planes, stride 1: the three depth taps inside ONE linear-pixel launch
  FWD_S2D,               // stride 2, small even planes: space-to-depth copy + ONE grouped-tap linear-pixel launch
  FWD_S2_TAPS,           // native stride-2 tiles, kd == 1
  FWD_S2_FUSED,          // native stride-2 tiles, the three depth taps inside ONE launch
  FWD_SUB,               // stride 2 without a strided kernel: FWD_TAPS into a scratch tensor + subsample
  FWD_BF16               // UNETK_BF16: ONE launch, the depth taps fused into its K loop
};
enum DgradRoute {
  DGRAD_NONE,            // refused
  DGRAD_GEN_DPAR,        // stride 2, four parity classes from the undilated dy: both depth parities of a (2,2,2) layer in ONE launch
  DGRAD_GEN_FUSED,       // ... the three depth taps of a (1,2,2) layer in ONE launch
  DGRAD_GEN_TAPS,        // ... one accumulating launch per depth tap
  DGRAD_FUSED_LIN,       // small planes, stride 1: as FWD_FUSED_LIN
  DGRAD_TAPS,            // one stride-1 launch per depth tap
  DGRAD_DILATED,         // stride 2 fallback: DGRAD_TAPS on the zero-dilated dy
  DGRAD_BF16             // as FWD_BF16
};
struct Tap { int dt, lo, hi; };      // depth tap dt reaches the output planes lo .. hi
struct Conv3dPlan {
  int rc;                // the layer itself: UNETK_E_BADARG (descriptor), UNETK_E_UNSUPPORTED (bf16 outside the layer rule)
  Geo3 g;
  int fwd, dgrad;        // FwdRoute, DgradRoute
  // what the descriptor decides against one op (`admit` below): UNETK_E_BADARG = a stride or channel multiple the route needs,
  // UNETK_E_UNSUPPORTED = no kernel for the channel counts (the route of a refused input gradient is DGRAD_NONE)
  int fwd_rc, dgrad_rc, wgrad_rc;
  Tap tap[3];            // the forward's per-tap routes: the launches in order, the full-coverage tap last (it emits the
  int ntaps;             // statistics); each is planned at its own plane count N * (hi - lo + 1), unetk_split is not monotone
  int stat_rows;         // rows of the launch that writes the statistics; rc where the layer is refused (bf16: or its launch's)
  WgRuns wg;             // the filter gradient's launches
  int klive_f, klive_b;  // live channels of the contraction axis, forward / input gradient (the stream-K cut is sized by them)
  // workspace.  Forward: FWD_SUB's stride-1 result in the first scratch_f floats; FWD_S2D's copy of x in the first xs_f, its
  // stream-K slab behind.  Input gradient: DGRAD_DILATED's dy in the first scratch_f floats; the fused-tap linear routes of
  // both directions take the whole workspace as slab.  Filter gradient: the dilated dy in the first wg.zf floats, the slabs
  // of the splits behind.
  size_t scratch_f, xs_f;
  size_t ws_bytes;
};

Conv3dPlan conv3d_plan(const unetk_conv3d_desc* d, int prec) {
  static const int s2lin = unetk_env_int("UNETK_S2LIN", 1);      // 0 (measurement): the routes before the s2d copy / dpar launch
  Conv3dPlan pl{};
  pl.rc = pl.stat_rows = UNETK_E_BADARG;
  if (!desc_ok(d)) return pl;
  const Geo3 g = pl.g = geo3(d);
  const bool s4 = d->x_stride % 4 == 0 && d->y_stride % 4 == 0;
  const int np = d->N * g.Do;
  if (prec == UNETK_BF16) {
    pl.rc = pl.stat_rows = UNETK_E_UNSUPPORTED;      // the layer rule (include/unetk.h)
    if (d->sd != 1 || d->shw != 1 || d->Cin % 32 != 0 || d->Cout % 32 != 0) return pl;
    pl.rc = UNETK_OK;
    pl.fwd = FWD_BF16; pl.dgrad = DGRAD_BF16;
    pl.fwd_rc = pl.dgrad_rc = pl.wgrad_rc = s4 ? UNETK_OK : UNETK_E_BADARG;
    const ConvPlan cp = plane_plan(np, d->H, d->W, d->Cin, d->Cout, d->D, 0, 0, 0, 1, UNETK_BF16);
    pl.stat_rows = cp.stat_rows > 0 ? cp.stat_rows : cp.rc;
    pl.wg = wg_runs(d, g, UNETK_BF16);
    pl.ws_bytes = wg_runs_bytes(pl.wg);
    return pl;
  }
  pl.rc = UNETK_OK;
  const bool s2 = d->shw == 2, taps3 = d->kd == 3 && d->sd == 1;      // taps3: every plane receives all three depth taps
  pl.klive_f = live_k(d->cin_live8, d->Cin);
  pl.klive_b = live_k(d->cout_live8, d->Cout);
  // ---- forward.  `out` = one launch over every output plane: its family admits the two linear-pixel routes, and its rows
  // are those of the per-tap routes' last launch (the full-coverage tap)
  const ConvPlan out = plane_plan(np, g.Ho, g.Wo, d->Cin, d->Cout, g.Do);
  pl.fwd_rc = d->y_stride % 4 == 0 ? UNETK_OK : UNETK_E_BADARG;
  pl.stat_rows = out.stat_rows;
  if (!s2 && taps3 && is_lin(out)) {
    pl.fwd = FWD_FUSED_LIN;
  } else if (s2lin && s2 && !(d->H & 1) && !(d->W & 1) && d->Cin % 16 == 0 && (d->sd == 1 || (!(d->D & 1) && d->kd == 3)) &&
             is_lin(out)) {
    // OUTPUT planes in the linear-pixel kernel's range (W < 32) and even input extents: SAME padding then puts the one pad
    // row / column / plane behind the data
    pl.fwd = FWD_S2D;
    pl.xs_f = ((size_t)np * g.Ho * g.Wo * (d->sd == 2 ? 8 : 4) * d->Cin + 63) & ~(size_t)63;
    if (d->x_stride % 4 != 0) pl.fwd_rc = UNETK_E_BADARG;
  } else if (s2 && unetk_conv_stride2_ok(d->Cin, d->Cout)) {
    pl.fwd = d->kd == 3 ? FWD_S2_FUSED : FWD_S2_TAPS;
    pl.stat_rows = plane_plan(np, g.Ho, g.Wo, d->Cin, d->Cout, g.Do, 0, 0, 0, 2).stat_rows;
  } else if (s2) {
    pl.fwd = FWD_SUB;
    pl.stat_rows = d->N * SUB_BPS;
    if (d->Cout % 4 != 0) pl.fwd_rc = UNETK_E_BADARG;
    else if (d->Cout > 1024 && pl.fwd_rc == UNETK_OK) pl.fwd_rc = UNETK_E_UNSUPPORTED;      // subsample2_stats_kernel's thread map
  } else {
    pl.fwd = FWD_TAPS;
  }
  if (pl.fwd == FWD_TAPS || pl.fwd == FWD_S2_TAPS || pl.fwd == FWD_SUB) {
    Tap full{-1, 0, 0};
    for (int dt = 0; dt < d->kd; ++dt) {
      Tap t{dt, 0, 0};
      tap_range(d, g, dt, &t.lo, &t.hi);
      if (full.dt < 0 && t.lo == 0 && t.hi == g.Do - 1) full = t;
      else if (t.hi >= t.lo) pl.tap[pl.ntaps++] = t;
    }
    if (full.dt >= 0) pl.tap[pl.ntaps++] = full;
    else if (pl.fwd_rc == UNETK_OK) pl.fwd_rc = UNETK_E_UNSUPPORTED;
  }
  // ---- input gradient: the conv of dy with Cin and Cout swapped
  if (!s4 || d->Cout % 4 != 0) pl.dgrad_rc = UNETK_E_BADARG;
  else if (d->Cout % 16 != 0 || d->Cin % 32 != 0) pl.dgrad_rc = UNETK_E_UNSUPPORTED;      // the MFMA kernels' K and N granularity
  else if (s2 && unetk_conv_lin_gen_ok(g.Ho, g.Wo, d->Cout, d->Cin))
    pl.dgrad = s2lin && d->kd == 3 && d->sd == 2 && !(d->D & 1) && g.pb_d == 0 ? DGRAD_GEN_DPAR
               : taps3                                                       ? DGRAD_GEN_FUSED
                                                                             : DGRAD_GEN_TAPS;
  else if (s2) pl.dgrad = DGRAD_DILATED;
  else pl.dgrad = taps3 && is_lin(plane_plan(np, d->H, d->W, d->Cout, d->Cin, d->D)) ? DGRAD_FUSED_LIN : DGRAD_TAPS;
  // ---- filter gradient
  pl.wg = wg_runs(d, g, UNETK_FP32);
  pl.wgrad_rc = d->y_stride % 4 == 0 ? UNETK_OK : UNETK_E_BADARG;
  // ---- workspace: one size serves the three ops
  if (s2) pl.scratch_f = ((size_t)np * d->H * d->W * d->Cout + 63) & ~(size_t)63;      // stride-1 result / dilated dy
  pl.ws_bytes = pl.scratch_f * sizeof(float);
  auto at_least = [&pl](size_t bytes) { if (bytes > pl.ws_bytes) pl.ws_bytes = bytes; };
  at_least(wg_runs_bytes(pl.wg));
  if (pl.fwd == FWD_S2D)
    at_least(pl.xs_f * sizeof(float) + plane_plan(np, g.Ho, g.Wo, d->Cin, d->Cout, g.Do, pl.klive_f, 0, d->kd * 4).ws_bytes);
  if (!s2 && d->sd == 1) {      // stream-K slabs of the small-plane kernel, forward and input gradient
    at_least(plane_plan(np, d->H, d->W, d->Cin, d->Cout, d->D, pl.klive_f, d->kd).ws_bytes);
    at_least(plane_plan(np, d->H, d->W, d->Cout, d->Cin, d->D, pl.klive_b, d->kd).ws_bytes);
  }
  return pl;
}

// The refusals of a call in the one order every entry point keeps: the layer, the arguments of the call and the multiples the
// op's route needs (UNETK_E_BADARG), the workspace where the route takes one, then the channel counts no kernel takes.
int admit(const Conv3dPlan& pl, bool args_ok, int op_rc, bool needs_ws, const void* ws, size_t ws_bytes) {
  if (pl.rc != UNETK_OK) return pl.rc;
  if (!args_ok || op_rc == UNETK_E_BADARG) return UNETK_E_BADARG;
  if (needs_ws) {
    if (!ws || !unetk_aligned16(ws)) return UNETK_E_BADARG;
    if (ws_bytes < pl.ws_bytes) return UNETK_E_WORKSPACE;
  }
  return op_rc;
}

// ---------------------------------------------------------------- the launchers
// A stride-1 layer in ONE launch over all its planes, forward (in = x, out = y) or input gradient (in = dy, out = dx, the
// channels swapped), the three depth taps inside the K loop -- no memset, no read-modify-write of the output per tap:
//   y[o] = sum_dt x[o - 1 + dt] w[dt],  dx[i] = sum_dt dy[i + 1 - dt] w'[dt]     (SAME pad-before of a (3,.,.) kernel is 1)
// fp32 (FWD / DGRAD_FUSED_LIN): the linear-pixel kernel on small planes (UNet3D's 24^2 / 12^2 / 6^2 levels), K = 27 Cin over
// the live channels, the whole workspace on offer as stream-K slab.  UNETK_BF16 (FWD / DGRAD_BF16): conv3x3_igemm_bf16_kernel,
// kd = 1 included
int run_fused(const unetk_conv3d_desc* d, int prec, bool fwd, const float* in, const float* wp, float* out, float* stat, void* ws,
              size_t ws_bytes, hipStream_t st) {
  const int Cin = fwd ? d->Cin : d->Cout, Cout = fwd ? d->Cout : d->Cin, is = fwd ? d->x_stride : d->y_stride;
  const int os = fwd ? d->y_stride : d->x_stride, HWi = d->H * d->W * is;
  ConvParams p = plane_params(in, wp, out, d->N * d->D, d->H, d->W, Cin, Cout, is, os, planes(HWi, d->D, 1, d->D),
                              planes(d->H * d->W * os, d->D, 1, d->D), d->D);
  p.stat = stat;
  if (d->kd == 3) { p.kd = 3; p.dshift0 = fwd ? -1 : 1; p.dstep = fwd ? 1 : -1; }
  if (prec == UNETK_BF16) {
    p.bf16 = UNETK_BF16;
    if (d->kd == 3) { p.dsd = 1; p.din = d->D; p.dplane = HWi; }
  } else {
    set_live(p, fwd ? d->cin_live8 : d->cout_live8, Cin);
    if (ws && unetk_aligned16(ws)) { p.sk_slab = (float*)ws; p.sk_slab_bytes = ws_bytes; }
  }
  return unetk_conv_run(p, st);
}

// The tap groups of a strided conv over the space-to-depth copy of its input (ConvParams::ng): group = (depth tap, in-plane class)
void set_s2d_groups(ConvParams& p, const unetk_conv3d_desc* d, const Geo3& g) {
  int ng = 0;
  for (int kd_ = 0; kd_ < d->kd; ++kd_) {
    const int cd = d->sd == 2 ? (kd_ & 1) : 0;
    const int dz = d->sd == 2 ? (kd_ >> 1) : kd_ - g.pb_d;      // depth stride 1: input plane = do + kd - pb
    for (int ph = 0; ph < 2; ++ph)
      for (int pw = 0; pw < 2; ++pw, ++ng) {
        p.g_chan[ng] = ((cd * 2 + ph) * 2 + pw) * d->Cin;
        p.g_dz[ng] = dz;
        int nt = 0;
        for (int kh = ph; kh < 3; kh += 2)
          for (int kw = pw; kw < 3; kw += 2, ++nt) {
            p.g_off[ng][nt] = 4 * ((kh >> 1) + 1) + ((kw >> 1) + 1);      // output o reads class k & 1 at o + (k >> 1)
            p.g_panel[ng][nt] = kd_ * 9 + kh * 3 + kw;
          }
        p.g_ntaps[ng] = nt;
      }
  }
  p.ng = ng;
}

// Small OUTPUT planes behind a stride-2 layer: space-to-depth copy of x into the workspace, then ONE launch of the linear-pixel
// kernel over kd x 4 tap groups (K = kd x 9 x Cin, every MFMA row an output pixel, stream-K in the workspace behind the copy)
int fwd_s2d(const unetk_conv3d_desc* d, const Conv3dPlan& pl, const float* x, const float* wp, float* y, float* stat, void* ws,
            size_t ws_bytes, hipStream_t st) {
  const Geo3& g = pl.g;
  float* XS = (float*)ws;
  const int ncls = d->sd == 2 ? 8 : 4;
  const int64_t npix_out = (int64_t)d->N * g.Do * g.Ho * g.Wo;
  UNETK_LAUNCH(s2d_kernel, dim3(ew_grid(npix_out * ncls * (d->Cin / 4))), dim3(256), 0, st, x, d->x_stride, XS, npix_out, g.Do, d->D,
               d->H, d->W, g.Ho, g.Wo, d->Cin, d->sd);
  UNETK_LAUNCH_CHECK();
  ConvParams p = plane_params(XS, wp, y, d->N * g.Do, g.Ho, g.Wo, d->Cin, d->Cout, ncls * d->Cin, d->y_stride,
                              planes(g.Ho * g.Wo * ncls * d->Cin, g.Do, 1, g.Do), planes(g.Ho * g.Wo * d->y_stride, g.Do, 1, g.Do), g.Do);
  p.stat = stat;
  set_s2d_groups(p, d, g);
  set_live(p, d->cin_live8, d->Cin);
  p.sk_slab = XS + pl.xs_f; p.sk_slab_bytes = ws_bytes - pl.xs_f * sizeof(float);
  return unetk_conv_run(p, st);
}

// Natively strided (3,3,3) conv (UNet3D's (1,2,2) and (2,2,2) down-sampling layers): the three depth taps are contracted inside
// ONE launch of the tiled stride-2 kernel (K = 27 Cin; a tap whose input plane falls outside the sample is skipped per block) --
// no memset, no read-modify-write of y per tap, one prologue / epilogue instead of three
int fwd_s2_fused(const unetk_conv3d_desc* d, const Conv3dPlan& pl, const float* x, const float* wp, float* y, float* stat, hipStream_t st) {
  const Geo3& g = pl.g;
  const int HWx = d->H * d->W * d->x_stride;
  ConvParams p = plane_params(x, wp, y, d->N * g.Do, g.Ho, g.Wo, d->Cin, d->Cout, d->x_stride, d->y_stride,
                              planes(HWx, g.Do, d->sd, d->D), planes(g.Ho * g.Wo * d->y_stride, g.Do, 1, g.Do), g.Do);
  p.stat = stat;
  p.stride = 2; p.Hin = d->H; p.Win = d->W; p.pbh = 1 - g.off_h; p.pbw = 1 - g.off_w;
  p.kd = 3; p.dshift0 = -g.pb_d; p.dstep = 1; p.dsd = d->sd; p.din = d->D; p.dplane = HWx;
  return unetk_conv_run(p, st);
}

// One launch per depth tap of pl.tap over the planes the tap reaches.  FWD_S2_TAPS: the tiled stride-2 kernel; FWD_SUB: the
// stride-1 result goes to the workspace, and the subsample kernel writes y and the statistics from it
int fwd_taps(const unetk_conv3d_desc* d, const Conv3dPlan& pl, const float* x, const float* wp, float* y, float* stat, void* ws,
             hipStream_t st) {
  const Geo3& g = pl.g;
  const bool native = pl.fwd == FWD_S2_TAPS, sub = pl.fwd == FWD_SUB;
  float* T = sub ? (float*)ws : y;
  const int ts = sub ? d->Cout : d->y_stride;
  const int Hp = native ? g.Ho : d->H, Wp = native ? g.Wo : d->W;      // the planes the launches write
  const int HWx = d->H * d->W * d->x_stride, HWt = Hp * Wp * ts;
  if (d->kd > 1) {
    const int zr = zero_pixels(T, (int64_t)d->N * g.Do * Hp * Wp, d->Cout, ts, st);
    if (zr != UNETK_OK) return zr;
  }
  for (int i = 0; i < pl.ntaps; ++i) {
    const Tap& t = pl.tap[i];
    const int n = t.hi - t.lo + 1;
    ConvParams p = plane_params(x + (int64_t)(t.lo * d->sd - g.pb_d + t.dt) * HWx, wp + (int64_t)t.dt * 9 * d->Cin * d->Cout,
                                T + (int64_t)t.lo * HWt, d->N * n, Hp, Wp, d->Cin, d->Cout, d->x_stride, ts,
                                planes(HWx, n, d->sd, d->D), planes(HWt, n, 1, g.Do), n);
    p.stat = (i == pl.ntaps - 1 && !sub) ? stat : nullptr;
    p.accumulate = d->kd > 1 ? 1 : 0;
    if (native) { p.stride = 2; p.Hin = d->H; p.Win = d->W; p.pbh = 1 - g.off_h; p.pbw = 1 - g.off_w; }
    const int rc = unetk_conv_run(p, st);
    if (rc != UNETK_OK) return rc;
  }
  if (sub) {
    const ColMap m = unetk_colmap(d->Cout);
    const size_t lds = stat ? (size_t)2 * m.rows_per_iter * d->Cout * sizeof(float) : 0;
    UNETK_LAUNCH(subsample2_stats_kernel, dim3(d->N * SUB_BPS), dim3(256), lds, st, T, y, stat, g.Do, d->H, d->W, g.Ho, g.Wo, d->Cout,
                 d->y_stride, g.off_h, g.off_w, m.cq_n, m.rows_per_iter, SUB_BPS, d->N * SUB_BPS);
    UNETK_LAUNCH_CHECK();
  }
  return UNETK_OK;
}

// wp: the fp32 pack, or the bf16 pack of the bf16 entry points
int conv3d_fwd(const unetk_conv3d_desc* d, int prec, const float* x, const float* wp, float* y, float* stat, void* ws, size_t ws_bytes,
               void* stream) {
  const Conv3dPlan pl = conv3d_plan(d, prec);
  const int rc = admit(pl, x && wp && y && unetk_aligned16(x) && unetk_aligned16(wp) && unetk_aligned16(y), pl.fwd_rc,
                       pl.fwd == FWD_SUB || pl.fwd == FWD_S2D || pl.fwd == FWD_BF16, ws, ws_bytes);
  if (rc != UNETK_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  switch (pl.fwd) {
    case FWD_FUSED_LIN:
    case FWD_BF16: return run_fused(d, prec, true, x, wp, y, stat, ws, ws_bytes, st);
    case FWD_S2D: return fwd_s2d(d, pl, x, wp, y, stat, ws, ws_bytes, st);
    case FWD_S2_FUSED: return fwd_s2_fused(d, pl, x, wp, y, stat, st);
    default: return fwd_taps(d, pl, x, wp, y, stat, ws, st);
  }
}

// dy -> (Z, stride) usable by the stride-1 backward kernels: dy itself, or (dilate) its zero-dilated copy in the first floats of ws
int dilated_dy(const unetk_conv3d_desc* d, const Geo3& g, bool dilate, const float* dy, void* ws, hipStream_t st, const float** z,
               int* zs) {
  *z = dy;
  *zs = d->y_stride;
  if (!dilate) return UNETK_OK;
  float* Z = (float*)ws;
  const size_t n = (size_t)d->N * g.Do * d->H * d->W * d->Cout;
  hipError_t e = hipMemsetAsync(Z, 0, n * sizeof(float), st);
  if (e != hipSuccess) return (int)e;
  const int64_t npix_out = (int64_t)d->N * g.Do * g.Ho * g.Wo;
  UNETK_LAUNCH(dilate2_kernel, dim3(ew_grid(npix_out * (d->Cout / 4))), dim3(256), 0, st, dy, d->y_stride, Z, npix_out, d->H, d->W,
               g.Ho, g.Wo, d->Cout, g.off_h, g.off_w);
  UNETK_LAUNCH_CHECK();
  *z = Z;
  *zs = d->Cout;
  return UNETK_OK;
}

// dx = 0 before the accumulating launches of a per-tap input gradient
int zero_dx(const unetk_conv3d_desc* d, float* dx, hipStream_t st) {
  return zero_pixels(dx, (int64_t)d->N * d->D * d->H * d->W, d->Cin, d->x_stride, st);
}

// The four output-parity classes of a stride-2 conv's input gradient (conv_igemm_lin.hip GEN), pbh / pbw = SAME pad-before:
//   dx[hi] = sum_{kh = ph, ph+2} dy[a - (kh - ph)/2] w[kh],  ph = (hi + pbh) & 1,  a = (hi + pbh - ph) / 2
// class q = 2 ph + pw contracts the undilated dy over its 4 / 2 / 2 / 1 taps
void set_parity_taps(ConvParams& p, int pbh, int pbw) {
  for (int ph = 0; ph < 2; ++ph)
    for (int pw = 0; pw < 2; ++pw) {
      const int q = ph * 2 + pw;
      p.ooh[q] = ph - pbh;
      p.oow[q] = pw - pbw;
      p.ntaps[q] = 0;
      for (int kh = ph; kh < 3; kh += 2)
        for (int kw = pw; kw < 3; kw += 2) {
          p.tap_off[q][p.ntaps[q]] = 4 * ((ph - kh) / 2 + 1) + ((pw - kw) / 2 + 1);
          p.tap_panel[q][p.ntaps[q]] = 8 - (kh * 3 + kw);
          ++p.ntaps[q];
        }
    }
}

// The three four-class routes.  DGRAD_GEN_FUSED (depth stride 1, UNet3D's (1,2,2) layers): every dx plane receives all three
// depth taps, contracted in ONE launch (K = 3 x taps x Cout) -- no memset, no accumulation passes.  DGRAD_GEN_DPAR (the (2,2,2)
// bridge): dx plane di = 2 do + dt (pad-before 0 for an even depth), so the EVEN dx planes receive the taps dt = 0 (do = di / 2)
// and dt = 2 (do = di / 2 - 1), the ODD ones dt = 1 alone -- both parities in ONE launch that writes every plane once.
// DGRAD_GEN_TAPS: one launch per depth tap, accumulating into a zeroed dx where more than one tap reaches a plane
int dgrad_gen(const unetk_conv3d_desc* d, const Conv3dPlan& pl, const float* dy, const float* wp, float* dx, hipStream_t st) {
  const Geo3& g = pl.g;
  const int HWx = d->H * d->W * d->x_stride, HWy = g.Ho * g.Wo * d->y_stride;
  const bool dpar = pl.dgrad == DGRAD_GEN_DPAR, fused = pl.dgrad == DGRAD_GEN_FUSED;
  const bool multi = pl.dgrad == DGRAD_GEN_TAPS && (d->kd > 1 || d->sd > 1);
  int rc = UNETK_OK;
  if (multi && (rc = zero_dx(d, dx, st)) != UNETK_OK) return rc;
  for (int dt = 0; dt < (dpar || fused ? 1 : d->kd); ++dt) {
    int lo = 0, hi = g.Do - 1;
    if (pl.dgrad == DGRAD_GEN_TAPS) tap_range(d, g, dt, &lo, &hi);
    if (hi < lo) continue;
    const int n = hi - lo + 1;
    ConvParams p = plane_params(dy + (int64_t)lo * HWy, wp + (int64_t)dt * 9 * d->Cin * d->Cout,
                                dx + (int64_t)(dpar || fused ? 0 : lo * d->sd - g.pb_d + dt) * HWx, d->N * n, g.Ho, g.Wo, d->Cout, d->Cin,
                                d->y_stride, d->x_stride, planes(HWy, n, 1, g.Do), planes(HWx, n, d->sd, d->D), n);
    p.accumulate = multi ? 1 : 0;
    if (fused) { p.kd = 3; p.dshift0 = g.pb_d; p.dstep = -1; }      // dx[di] = sum_dt dy[di + pb - dt] * w[dt]
    if (dpar) {
      p.dshift0 = 0; p.dstep = -1;            // even planes: dy plane do = di / 2 - dt' for the fused taps dt' = 0, 1 (dt = 0, 2)
      p.dpar = 1; p.dpar_yoff = HWx;          // odd planes: one plane further
    }
    set_live(p, d->cout_live8, d->Cout);
    p.os = 2; p.Hd = d->H; p.Wd = d->W;
    set_parity_taps(p, 1 - g.off_h, 1 - g.off_w);
    if ((rc = unetk_conv_run_lin_gen(p, st)) != UNETK_OK) return rc;
  }
  return UNETK_OK;
}

// DGRAD_TAPS / DGRAD_DILATED: one stride-1 launch per depth tap, dy planes lo .. hi -> dx planes di = do * sd - pb + dt
int dgrad_taps(const unetk_conv3d_desc* d, const Conv3dPlan& pl, const float* dy, const float* wp, float* dx, void* ws, hipStream_t st) {
  const Geo3& g = pl.g;
  const float* Z;
  int zs;
  int rc = dilated_dy(d, g, pl.dgrad == DGRAD_DILATED, dy, ws, st, &Z, &zs);
  if (rc != UNETK_OK) return rc;
  const int HWx = d->H * d->W * d->x_stride, HWz = d->H * d->W * zs;
  const bool multi = d->kd > 1 || d->sd > 1;
  if (multi && (rc = zero_dx(d, dx, st)) != UNETK_OK) return rc;
  for (int dt = 0; dt < d->kd; ++dt) {
    int lo, hi;
    tap_range(d, g, dt, &lo, &hi);
    if (hi < lo) continue;
    const int n = hi - lo + 1;
    ConvParams p = plane_params(Z + (int64_t)lo * HWz, wp + (int64_t)dt * 9 * d->Cin * d->Cout,
                                dx + (int64_t)(lo * d->sd - g.pb_d + dt) * HWx, d->N * n, d->H, d->W, d->Cout, d->Cin, zs, d->x_stride,
                                planes(HWz, n, 1, g.Do), planes(HWx, n, d->sd, d->D), n);
    p.accumulate = multi ? 1 : 0;
    rc = unetk_conv_run(p, st);
    if (rc != UNETK_OK) return rc;
  }
  return UNETK_OK;
}

int conv3d_dgrad(const unetk_conv3d_desc* d, int prec, const float* dy, const float* wp, float* dx, void* ws, size_t ws_bytes,
                 void* stream) {
  const Conv3dPlan pl = conv3d_plan(d, prec);
  const int rc = admit(pl, dy && wp && dx && unetk_aligned16(dy) && unetk_aligned16(wp) && unetk_aligned16(dx), pl.dgrad_rc,
                       pl.dgrad == DGRAD_DILATED || pl.dgrad == DGRAD_BF16, ws, ws_bytes);
  if (rc != UNETK_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  switch (pl.dgrad) {
    case DGRAD_GEN_DPAR:
    case DGRAD_GEN_FUSED:
    case DGRAD_GEN_TAPS: return dgrad_gen(d, pl, dy, wp, dx, st);
    case DGRAD_FUSED_LIN:
    case DGRAD_BF16: return run_fused(d, prec, false, dy, wp, dx, nullptr, ws, ws_bytes, st);
    default: return dgrad_taps(d, pl, dy, wp, dx, ws, st);
  }
}

// ---------------------------------------------------------------- filter gradient
// Z, zs: dy and its pixel stride (dilated where r.zf); ws: behind the dilated dy
int run_wgrad(const unetk_conv3d_desc* d, const Geo3& g, const WgRuns& r, const float* x, const float* Z, int zs, float* dw,
              void* ws, size_t ws_bytes, hipStream_t st) {
  const int HWx = d->H * d->W * d->x_stride;
  for (int i = 0; i < r.n; ++i) {
    const WgRun& t = r.run[i];
    const int np = t.hi - t.lo + 1, HWz = t.s.H * t.s.W * zs;
    float* dw_t = dw + (int64_t)(t.dt < 0 ? 0 : t.dt) * 9 * d->Cin * d->Cout;
    if (np <= 0) {
      hipError_t e = hipMemsetAsync(dw_t, 0, (size_t)9 * d->Cin * d->Cout * sizeof(float), st);
      if (e != hipSuccess) return (int)e;
      continue;
    }
    WgParams p{};
    p.x = x; p.dy = Z + (int64_t)t.lo * HWz;
    p.N = t.s.N; p.H = t.s.H; p.W = t.s.W; p.Cin = d->Cin; p.Cout = d->Cout;
    p.xs = d->x_stride; p.ys = zs;
    p.bf16 = t.s.prec;
    if (r.native) { p.stride = 2; p.Hin = d->H; p.Win = d->W; p.pbh = same_pb(d->H, 3, 2); p.pbw = same_pb(d->W, 3, 2); }
    p.xa = planes(HWx, np, d->sd, d->D);
    p.ya = planes(HWz, np, 1, g.Do);
    if (t.dt < 0) {      // every dy plane against the x plane each tap reads
      p.kd = 3; p.dshift0 = -g.pb_d; p.dsd = d->sd; p.din = d->D; p.spg = g.Do; p.dplane = HWx;
    } else {
      p.x += (int64_t)(t.lo * d->sd - g.pb_d + t.dt) * HWx;
    }
    const int rc = unetk_wgrad_run(p, dw_t, ws, ws_bytes, st);
    if (rc != UNETK_OK) return rc;
  }
  return UNETK_OK;
}

int conv3d_wgrad(const unetk_conv3d_desc* d, int prec, const float* x, const float* dy, float* dw, void* ws, size_t ws_bytes,
                 void* stream) {
  const Conv3dPlan pl = conv3d_plan(d, prec);
  int rc = admit(pl, x && dy && dw && unetk_aligned16(x) && unetk_aligned16(dy) && unetk_aligned16(dw), pl.wgrad_rc, true, ws, ws_bytes);
  if (rc != UNETK_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const float* Z;
  int zs;
  if ((rc = dilated_dy(d, pl.g, pl.wg.zf != 0, dy, ws, st, &Z, &zs)) != UNETK_OK) return rc;
  return run_wgrad(d, pl.g, pl.wg, x, Z, zs, dw, (float*)ws + pl.wg.zf, ws_bytes - pl.wg.zf * sizeof(float), st);
}

}  // namespace

extern "C" int unetk_conv3d_pack(const float* w, int kd, int Cin, int Cout, float* wp_fwd, float* wp_dgrad,
                                 void* stream) {
  UNETK_REQUIRE(w && (kd == 1 || kd == 3) && Cin > 0 && Cout > 0);
  for (int dt = 0; dt < kd; ++dt) {
    const int64_t o = (int64_t)dt * 9 * Cin * Cout;
    int rc = unetk_conv3x3_pack(w + o, Cin, Cout, wp_fwd ? wp_fwd + o : nullptr, wp_dgrad ? wp_dgrad + o : nullptr, stream);
    if (rc != UNETK_OK) return rc;
  }
  return UNETK_OK;
}

extern "C" int unetk_conv3d_out_dims(const unetk_conv3d_desc* d, int* Do, int* Ho, int* Wo) {
  const Conv3dPlan pl = conv3d_plan(d, UNETK_FP32);
  if (pl.rc != UNETK_OK) return pl.rc;
  if (Do) *Do = pl.g.Do;
  if (Ho) *Ho = pl.g.Ho;
  if (Wo) *Wo = pl.g.Wo;
  return UNETK_OK;
}

extern "C" int unetk_conv3d_stat_rows(const unetk_conv3d_desc* d) { return conv3d_plan(d, UNETK_FP32).stat_rows; }
extern "C" size_t unetk_conv3d_ws_bytes(const unetk_conv3d_desc* d) { return conv3d_plan(d, UNETK_FP32).ws_bytes; }

extern "C" int unetk_conv3d_fwd(const unetk_conv3d_desc* d, const float* x, const float* wp, float* y,
                                float* stat_partials, void* ws, size_t ws_bytes, void* stream) {
  return conv3d_fwd(d, UNETK_FP32, x, wp, y, stat_partials, ws, ws_bytes, stream);
}
extern "C" int unetk_conv3d_dgrad(const unetk_conv3d_desc* d, const float* dy, const float* wp_dgrad, float* dx,
                                  void* ws, size_t ws_bytes, void* stream) {
  return conv3d_dgrad(d, UNETK_FP32, dy, wp_dgrad, dx, ws, ws_bytes, stream);
}
extern "C" int unetk_conv3d_wgrad(const unetk_conv3d_desc* d, const float* x, const float* dy, float* dw, void* ws,
                                  size_t ws_bytes, void* stream) {
  return conv3d_wgrad(d, UNETK_FP32, x, dy, dw, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------- UNETK_BF16: the stride-1 3-D convs on the bf16 matrix cores
// (include/unetk.h: the layer rule).  Forward / input gradient: ONE launch of conv3x3_igemm_bf16_kernel per conv, the kd depth
// taps fused into its K loop (FT); filter gradient: ONE launch of the bf16 conv3x3_wgrad_kernel with WgParams::kd = kd, fixed
// splits + fixed-order slab reduction.  Every entry point takes the workspace of unetk_conv3d_ws_bytes_bf16 and refuses a
// missing, misaligned or short one.
extern "C" int unetk_conv3d_pack_bf16(const float* w, int kd, int Cin, int Cout, void* wp_fwd, void* wp_dgrad, void* stream) {
  UNETK_REQUIRE(w && (kd == 1 || kd == 3) && Cin > 0 && Cout > 0 && (wp_fwd || wp_dgrad));
  if (Cin % 32 != 0 || Cout % 32 != 0) return UNETK_E_UNSUPPORTED;
  UNETK_REQUIRE((!wp_fwd || unetk_aligned16(wp_fwd)) && (!wp_dgrad || unetk_aligned16(wp_dgrad)));
  for (int dt = 0; dt < kd; ++dt) {
    const int64_t o = (int64_t)dt * 9 * Cin * Cout;         // elements per depth tap: floats of w, bf16 of the packs
    const int rc = unetk_conv3x3_pack_bf16(w + o, Cin, Cout, wp_fwd ? (void*)((bf16_t*)wp_fwd + o) : nullptr,
                                           wp_dgrad ? (void*)((bf16_t*)wp_dgrad + o) : nullptr, stream);
    if (rc != UNETK_OK) return rc;
  }
  return UNETK_OK;
}

extern "C" int unetk_conv3d_stat_rows_bf16(const unetk_conv3d_desc* d) { return conv3d_plan(d, UNETK_BF16).stat_rows; }
extern "C" size_t unetk_conv3d_ws_bytes_bf16(const unetk_conv3d_desc* d) { return conv3d_plan(d, UNETK_BF16).ws_bytes; }

extern "C" int unetk_conv3d_fwd_bf16(const unetk_conv3d_desc* d, const float* x, const void* wp_fwd, float* y,
                                     float* stat_partials, void* ws, size_t ws_bytes, void* stream) {
  return conv3d_fwd(d, UNETK_BF16, x, (const float*)wp_fwd, y, stat_partials, ws, ws_bytes, stream);
}
extern "C" int unetk_conv3d_dgrad_bf16(const unetk_conv3d_desc* d, const float* dy, const void* wp_dgrad, float* dx,
                                       void* ws, size_t ws_bytes, void* stream) {
  return conv3d_dgrad(d, UNETK_BF16, dy, (const float*)wp_dgrad, dx, ws, ws_bytes, stream);
}
extern "C" int unetk_conv3d_wgrad_bf16(const unetk_conv3d_desc* d, const float* x, const float* dy, float* dw, void* ws,
                                       size_t ws_bytes, void* stream) {
  return conv3d_wgrad(d, UNETK_BF16, x, dy, dw, ws, ws_bytes, stream);
}
