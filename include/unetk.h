/*
 * unetk.h -- C ABI of libunetk.so: hand-written HIP (gfx950 / MI355X) kernels for the
 * U-Net conv encoder/decoder + loss-head hot path of Jarvis73/BoxSegLiver.
 *
 * The reference has NO native boundary for this path (it is pure Python on
 * tensorflow-gpu 1.13).  Each entry point below therefore cites the
 * reference *call site* whose TensorFlow op it replaces (paths relative to the
 * reference repo root).
 *
 * Conventions
 *   - all tensors are device pointers, fp32, NHWC, densely packed unless a
 *     "*_stride" (pixel stride, in ELEMENTS) argument says otherwise; labels int32.
 *     Activation tensors passed as `void*` are fp32, or bf16 (2 bytes / element) when the
 *     descriptor selects UNETK_BF16S ("bf16 storage", see below)
 *   - conv filters are TF HWIO [kh,kw,Cin,Cout]; transposed-conv filters are TF
 *     [kh,kw,Cout,Cin]  (slim.conv2d / slim.conv2d_transpose variable layouts)
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on it
 *   - no allocation, no host sync, no global mutable state: caller owns all buffers,
 *     including workspaces sized by the *_ws_bytes() queries  (graph-capturable)
 *   - return 0 on success, else a negative UNETK_E_* or a positive hipError_t
 *
 * Non-finite values on the forward path.  Training watches the LOSS only (unetk_nan_watch, as the reference's
 * NanTensorHook), so a NaN anywhere in front of the head has to reach the loss instead of turning into a finite number:
 *   1. ReLU: relu(NaN) = NaN.  Every other input, +-Inf included, gives max(v, 0); the sign of a zero result is not
 *      specified.  (fmaxf(NaN, 0) is 0: the forward kernels use unetk_relu of csrc/common.h, never fmaxf.)
 *   2. Max-pool (2x2, the fused norm+ReLU+pool and conv+affine+ReLU+pool epilogues, maxpool1d): a window that holds a NaN
 *      gives NaN, as F.max_pool2d / F.max_pool1d.  Finite windows are unchanged, and so is the backward tie rule (the first
 *      maximum takes the gradient; a NaN maximum equals no element, so the last element of its window takes it).
 *   3. Everything else (matrix kernels, statistic partials, norm_finalize, deconv, conv1d, fc, the head): a NaN operand
 *      reaches every output whose in-image receptive field holds it, by IEEE arithmetic; there is no fast-math flag in
 *      the build.  Whether a NaN FILTER tap reaches an output whose tap lies in the zero halo is not specified.
 *   4. Live-channel masks (cin_live8 / cout_live8 of unetk_conv3d_desc): padded channels are skipped, so 0 * NaN from a
 *      dead channel is NOT formed and a NaN there does not propagate.  The promise that pads are zero makes this
 *      unobservable; a caller that breaks the promise gets neither the product nor the NaN.
 * The backward ReLU gates (u > 0 ? d : 0) send a NaN pre-activation's gradient to 0: once the forward is NaN the step is
 * already refused.  fmaxf / fminf that remain and why they are safe: the softmax shift of the head (head.hip: expf(NaN -
 * mx) carries the NaN whatever mx is) and its union count fminf(pr + lc, 1) (both operands are 0 or 1); the re-evaluation
 * of z and of its window maximum in the pool-fused norm BACKWARD (norm.hip pool_window: it only routes dp inside a window,
 * on finite values it equals the forward's, and it runs after a forward whose NaN has refused the step); the intensity
 * clamp, min / max reductions and guide renderers of the LiTS loaders (lits.hip, lits3d.hip: their sources are uint16
 * volumes and host-made tables, not activations).
 */
#ifndef UNETK_H_
#define UNETK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNETK_OK 0
#define UNETK_E_BADARG (-1)       /* null pointer / non-positive size / misaligned */
#define UNETK_E_UNSUPPORTED (-2)  /* valid request this build has no kernel for */
#define UNETK_E_WORKSPACE (-3)    /* workspace too small */

#define UNETK_MAX_CLASSES 8

/* loss head weight modes: loss_metrics.py:115-165 `_compute_weights` w_type */
#define UNETK_W_NONE 0
#define UNETK_W_NUMERICAL 1
#define UNETK_W_PROPORTION 2
#define UNETK_W_PIXELMAP 3 /* caller-provided per-pixel map (covers `boundary`, which the
                              reference computes on the host via py_func, :149-159) */

/* loss types: loss_metrics.py:42-45 --loss_type */
#define UNETK_LOSS_XENTROPY 1
#define UNETK_LOSS_DICE 2

int unetk_abi_version(void);
const char* unetk_error_string(int code);

/* ---------------------------------------------------------------- conv 3x3 (slim.conv2d(x, C, 3))
 * NetworksV2/UNet.py:79,85,94 -- stride 1, SAME, no bias (a normaliser follows).
 * Geometry: x [N,H,W,Cin] (pixel stride x_stride >= Cin), y [N,H,W,Cout] (pixel stride y_stride). */
typedef struct unetk_conv_desc {
  int32_t N, H, W, Cin, Cout;
  int32_t x_stride, y_stride;
  int32_t precision; /* UNETK_FP32 (exact fp32 MFMA), UNETK_BF16, or UNETK_BF16S (x / y / dy / dx are bf16) */
  int32_t dilation;  /* 0 / 1 = dense 3x3; 2 = slim.conv2d(..., rate=2) (SmallUNet.py:44-49: bridge, conv_d3/conv1):
                        taps at (2 kh, 2 kw), SAME pads 2.  fp32 only, Cin % 16 == 0 and Cout % 64 == 0 (wgrad: both % 64) */
} unetk_conv_desc;

/* Arithmetic of the dense contractions.  UNETK_FP32: v_mfma_f32_32x32x2_f32, bit-for-bit an fp32 fmaf chain.
 * UNETK_BF16 (BASELINE.json configs[2], "bf16"): both operands rounded to bf16 (RNE) on their way into the
 * matrix cores (v_mfma_f32_32x32x16_bf16), fp32 accumulation, fp32 tensors in memory, fp32 statistics, master
 * weights and optimiser.  Needs Cin % 32 == 0 and Cout % 32 == 0 (else UNETK_E_UNSUPPORTED: use UNETK_FP32 for
 * that layer) and filters packed by unetk_conv3x3_pack_bf16.  The 3-D convs have the same contract through the
 * unetk_conv3d_*_bf16 entry points; their layer rule (stride 1, Cin % 32 == 0, Cout % 32 == 0, kd in {1, 3}) is
 * stated with them below. */
#define UNETK_FP32 0
#define UNETK_BF16 1
/* UNETK_BF16S = UNETK_BF16 arithmetic + bf16 STORAGE of activations and activation gradients (BASELINE.json
 * configs[2]: "bf16 activations / weights-compute, fp32 master / accum / stats"): every tensor passed as `void*`
 * (conv / deconv inputs and outputs, the norm's y / z / dz / dy, pooling, the head's feature map and its gradient)
 * is bf16 in memory, rounded RNE from the fp32 accumulator by the kernel that produces it; statistics come from the
 * fp32 accumulators, master weights, weight gradients, norm parameters and the optimiser stay fp32.  Halves the
 * bytes of every HBM-bound pass and lets the filter gradient read its k-strided operands with ds_read_b64_tr_b16.
 * The first conv (Cin < 16, direct kernel) reads fp32 images and writes bf16.  2-D, stride 1, dilation 1 only. */
#define UNETK_BF16S 2

/* Re-layout HWIO filters for the MFMA kernels ("K4-interleaved": [tap][Cin/4][Cout][4]).
 * wp_fwd feeds unetk_conv3x3_fwd; wp_dgrad (taps flipped, Cin<->Cout swapped) feeds
 * unetk_conv3x3_dgrad.  Either output may be NULL.  Each holds 9*Cin*Cout floats. */
int unetk_conv3x3_pack(const float* w_hwio, int Cin, int Cout, float* wp_fwd, float* wp_dgrad,
                       void* stream);

/* Every filter re-layout of a step in ONE launch.  An item = one filter tap-set: kind (which of the four packs above /
 * below), perm (1 = the UNETK_BF16S channel-pair permutation), Cin, Cout, the TF-layout source w and the two outputs
 * (either may be NULL), and the item's block range [block0, block0 + nblocks) inside the launch (nblocks from
 * unetk_pack_item_blocks, block0 = running sum; items ascending).  `items_dev` is the table in DEVICE memory (16-byte
 * aligned), total_blocks the sum of nblocks.  A 3-D filter is kd items (one per depth tap). */
#define UNETK_PACK_CONV3X3_F32 0   /* unetk_conv3x3_pack */
#define UNETK_PACK_CONV3X3_BF16 1  /* unetk_conv3x3_pack_bf16 (perm 0) / _bf16s (perm 1) */
#define UNETK_PACK_DECONV_F32 2    /* one depth tap of unetk_deconv3d_pack / unetk_deconv2x2_pack */
#define UNETK_PACK_DECONV_BF16 3   /* ... of the bf16 transposed-conv packs */
typedef struct {
  int32_t kind, perm, Cin, Cout, block0, nblocks, reserved0, reserved1;
  const void* w;
  void* wp_fwd;
  void* wp_dgrad;
  void* reserved2;
} unetk_pack_item;
int unetk_pack_item_blocks(int kind, int Cin, int Cout);
int unetk_pack_many(const unetk_pack_item* items_dev, int n_items, int total_blocks, void* stream);

/* UNETK_BF16 filters: bf16 "K8-interleaved" [tap][Cin/8][Cout][8]; each output holds 9*Cin*Cout bf16
 * (2 bytes each), 16-byte aligned.  Cin % 8 == 0 and Cout % 8 == 0. */
int unetk_conv3x3_pack_bf16(const float* w_hwio, int Cin, int Cout, void* wp_fwd, void* wp_dgrad,
                            void* stream);

/* UNETK_BF16S filters: as unetk_conv3x3_pack_bf16, with the OUTPUT channels of each pack (Cout for wp_fwd, Cin for
 * wp_dgrad) permuted inside every 64-channel block -- column position n' holds channel 2 (n' & 31) + (n' >> 5 & 1) -- so
 * that a lane of the bf16-storage kernels owns two adjacent channels and stores them as one word.  Cin % 64 == 0 and
 * Cout % 64 == 0. */
int unetk_conv3x3_pack_bf16s(const float* w_hwio, int Cin, int Cout, void* wp_fwd, void* wp_dgrad,
                             void* stream);

/* Number of per-channel statistic partial rows unetk_conv3x3_fwd writes (one per pixel tile). */
int unetk_conv3x3_stat_rows(const unetk_conv_desc* d);

/* y = conv3x3(x, w).  If stat_partials != NULL also writes per-pixel-tile partial sums for the
 * following norm: stat_partials[0][row][c] = sum y, stat_partials[1][row][c] = sum y^2
 * (2 * stat_rows * Cout floats; deterministic, no atomics).
 * `w` is wp_fwd from unetk_conv3x3_pack when Cin % 16 == 0 && Cout % 32 == 0, else the raw
 * HWIO filter (direct kernel; used by Encode1/conv1 where Cin = 3). */
int unetk_conv3x3_fwd(const unetk_conv_desc* d, const void* x, const void* w, void* y,
                      float* stat_partials, void* stream);

/* dx = conv3x3_input_grad(dy, w): d describes the FORWARD conv (dx has Cin channels,
 * pixel stride x_stride; dy has Cout channels, pixel stride y_stride).  `w` = wp_dgrad. */
int unetk_conv3x3_dgrad(const unetk_conv_desc* d, const void* dy, const void* w, void* dx,
                        void* stream);

/* unetk_conv3x3_fwd / _dgrad with a scratch buffer: small planes whose tile grid cannot fill the 256 CUs (the 16 x 16 bridge
 * of a 2-D net at 8 slices per GPU) are scheduled stream-K -- the (tile, K-chunk) sequence split evenly over the blocks,
 * pieces of split tiles summed in a fixed order from ws (deterministic).  unetk_conv3x3_ws_bytes = bytes the two calls may
 * use for this shape (0 = never); ws = NULL behaves as the plain entry points. */
size_t unetk_conv3x3_ws_bytes(const unetk_conv_desc* d);
int unetk_conv3x3_fwd_ws(const unetk_conv_desc* d, const void* x, const void* w, void* y, float* stat_partials,
                         void* ws, size_t ws_bytes, void* stream);
int unetk_conv3x3_dgrad_ws(const unetk_conv_desc* d, const void* dy, const void* w, void* dx, void* ws,
                           size_t ws_bytes, void* stream);

/* Inference (mode == EVAL, NetworksV2/base.py:71-79: is_training False -> slim.batch_norm uses the moving statistics;
 * --without_norm: conv + bias + ReLU, UNet.py:47-48): the normaliser's per-channel affine is known BEFORE the conv runs, so
 * the conv, slim.batch_norm and ReLU of one slim.conv2d(x, C, 3) -- and, when the unit feeds one, slim.max_pool2d(z, 2, 2)
 * (UNet.py:81) -- are ONE pass: z = relu(conv(x, w) * scale[c] + shift[c]) is written straight to z (pixel stride
 * d->y_stride: a channel slice of the decoder's concat buffer), the raw conv output never reaches memory.  SURVEY.md 7
 * step 2 / 8b: the conv forward taking (scale, shift).  scale / shift: [Cout] floats (unetk_norm_finalize rows 2, 3).
 * pooled != NULL: also pooled[N, H/2, W/2, .] (pixel stride pooled_stride) = max over each 2 x 2 window of z; H, W even.
 * ws / ws_bytes: the stream-K scratch of unetk_conv3x3_ws_bytes (small planes), may be NULL / 0.
 * unetk_conv3x3_fwd_affine_ok = 1 when the shape has the fused kernel (fp32: the tiled kernels, the Cout = 64 first layers
 * and -- without the pool -- the small-plane linear-pixel kernel; not strided or atrous convs, not the generic direct
 * kernel) -- else the caller runs conv + unetk_norm_apply_relu. */
int unetk_conv3x3_fwd_affine_ok(const unetk_conv_desc* d, int with_pool);
int unetk_conv3x3_fwd_affine(const unetk_conv_desc* d, const void* x, const void* w, const float* scale,
                             const float* shift, void* z, void* pooled, int pooled_stride, void* ws, size_t ws_bytes,
                             void* stream);

/* The same input gradient, fused with the norm-backward REDUCTION of the unit that produced the conv's input (the
 * slim.repeat(x, 2, slim.conv2d, ...) pairs of UNet.py:79,85,94: conv2's dx is the dz of conv1's norm + ReLU): while the
 * dx tile is in registers the epilogue reads prod_y (conv1's raw output, same [N,H,W,Cin], pixel stride prod_y_stride;
 * bf16 under UNETK_BF16S) and writes, per tile, the partial sums  sum du  and  sum du * xhat  (du = dx * (prod_y * scale +
 * shift > 0), xhat = (prod_y - mean) * rstd; scale / shift / mean / rstd are conv1's unetk_norm_finalize outputs,
 * [N][Cin] when per_sample else [Cin]) into partials [2][rows][Cin] -- the input unetk_norm_relu_bwd_pre takes instead of
 * running its own pass over (dz, y).  unetk_conv3x3_dgrad_nbr_rows = rows, or 0 when the shape has no fused variant
 * (tiled fp32 kernel and bf16-storage kernel only; the caller then uses the two separate calls).
 * Alignment of prod_y (dy, w, dx: 16 bytes, as for unetk_conv3x3_dgrad): the base address a multiple of 4 bytes in both
 * modes; under UNETK_BF16S prod_y_stride even (two bf16 channels are read as one word), and where the persistent kernel runs
 * -- H >= 24, at least 200 tiles of 32 x 16 pixels x 128 channels, x_stride / y_stride / prod_y_stride % 8 == 0 -- the base
 * a multiple of 16 bytes (a stride that is not a multiple of 8 is routed to the tall tile, which reads words).  Anything
 * else: UNETK_E_BADARG, nothing launched. */
int unetk_conv3x3_dgrad_nbr_rows(const unetk_conv_desc* d);
int unetk_conv3x3_dgrad_nbr(const unetk_conv_desc* d, const void* dy, const void* w, void* dx, const void* prod_y,
                            int prod_y_stride, const float* scale, const float* shift, const float* mean,
                            const float* rstd, int per_sample, float* partials, void* stream);

/* dw[HWIO] = conv3x3_filter_grad(x, dy).  Split-K over pixel tiles through a workspace of
 * fixed-order partial slabs (bit-reproducible).  The query is exact for the launch the descriptor names, its precision and
 * dilation included (256 + splits x 9 x Cin x Cout x 4 bytes), and 0 where the launch is refused: ask with the descriptor
 * you will run. */
size_t unetk_conv3x3_wgrad_ws_bytes(const unetk_conv_desc* d);
int unetk_conv3x3_wgrad(const unetk_conv_desc* d, const void* x, const void* dy, float* dw,
                        void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- slim.conv3d  (NetworksV2/UNet3D.py:153,165)
 * Kernels (1,3,3) / (3,3,3) from _ModelConfig (UNet3D.py:31-91), strides 1 / (1,2,2) / (2,2,2), TF SAME
 * padding (asymmetric at stride 2 on even sizes: 0 before, 1 after), no bias.
 * x [N,D,H,W,Cin] (pixel stride x_stride), y [N,Do,Ho,Wo,Cout] (pixel stride y_stride), Do = ceil(D/sd), ...
 * Filters: TF DHWIO [kd,3,3,Cin,Cout]; packed per depth tap like unetk_conv3x3_pack. */
typedef struct unetk_conv3d_desc {
  int32_t N, D, H, W, Cin, Cout;
  int32_t kd;   /* 1 or 3 */
  int32_t sd;   /* depth stride 1 or 2 (kd == 3 only) */
  int32_t shw;  /* H and W stride, 1 or 2 */
  int32_t x_stride, y_stride;
  /* Channel-padded nets (UNet3D's 30/60/120/240 real channels inside 32/64/128/256; ABI 10): bit i of the 64-bit mask
   * {lo, hi} = channels [8 i, 8 i + 8) of x (cin_live8) / of y (cout_live8) hold a real channel.  A promise by the caller that
   * the filter is ZERO in every other input row / output column: the forward then skips the dead groups of its contraction over
   * Cin, the input gradient those of its contraction over Cout (small-plane kernel; results equal to contracting the zeros).
   * 0 = no information, every channel is contracted. */
  uint32_t cin_live8[2], cout_live8[2];
} unetk_conv3d_desc;

int unetk_conv3d_pack(const float* w, int kd, int Cin, int Cout, float* wp_fwd, float* wp_dgrad,
                      void* stream);
int unetk_conv3d_out_dims(const unetk_conv3d_desc* d, int* Do, int* Ho, int* Wo);
int unetk_conv3d_stat_rows(const unetk_conv3d_desc* d);      /* rows of the statistic partials the forward writes */
size_t unetk_conv3d_ws_bytes(const unetk_conv3d_desc* d);    /* one size serves fwd / dgrad / wgrad */
/* Forward workspace: an H/W-strided conv (shw == 2) takes ws of at least unetk_conv3d_ws_bytes bytes, 16-byte aligned, and on
 * every path that uses it (stride-1 conv + subsample; space-to-depth copy for small output planes) a NULL or misaligned ws is
 * UNETK_E_BADARG and a short one UNETK_E_WORKSPACE -- the forward never falls back to a kernel that writes another number of
 * statistic rows than unetk_conv3d_stat_rows.  The space-to-depth path also needs x_stride % 4 == 0.  Stride 1 accepts ws = NULL. */
int unetk_conv3d_fwd(const unetk_conv3d_desc* d, const float* x, const float* wp_fwd, float* y,
                     float* stat_partials, void* ws, size_t ws_bytes, void* stream);
int unetk_conv3d_dgrad(const unetk_conv3d_desc* d, const float* dy, const float* wp_dgrad, float* dx,
                       void* ws, size_t ws_bytes, void* stream);
int unetk_conv3d_wgrad(const unetk_conv3d_desc* d, const float* x, const float* dy, float* dw,
                       void* ws, size_t ws_bytes, void* stream);

/* UNETK_BF16 for the 3-D convs (UNet3D --compute_dtype bf16c): the arithmetic contract of UNETK_BF16 above -- both operands
 * of every contraction rounded to bf16 (RNE) on their way into the matrix cores, fp32 accumulation, every tensor in memory
 * fp32, statistics, master weights, weight gradients and the optimiser fp32.  The entry points below imply it.
 * Layer rule (fixed): a conv runs on the bf16 pipe when it has stride 1 in all three axes, Cin % 32 == 0 and Cout % 32 == 0
 * (padded channels: 30 -> 32 qualifies) and kd in {1, 3}.  Every other descriptor gets UNETK_E_UNSUPPORTED and keeps the
 * exact fp32 entry points: in UNet3D the first conv (Cin = 1) and the four strided convs (about 11 % of the FLOPs).
 * Forward and input gradient contract K = kd x 9 x Cin (resp. Cout) in ONE launch, the depth taps fused; the filter gradient
 * is ONE launch over all kd taps with a fixed split and a fixed-order slab reduction (bit-reproducible, no atomics).
 * Filters: kd per-depth-tap bf16 K8 packs, each the layout of unetk_conv3x3_pack_bf16 (perm 0); the cin_live8 / cout_live8
 * promise is accepted and not needed (the padded rows are zero in the packs and contract to exactly 0).
 * ws / ws_bytes: at least unetk_conv3d_ws_bytes_bf16 bytes, 16-byte aligned, for all three calls: a NULL or misaligned ws
 * is UNETK_E_BADARG, a short one UNETK_E_WORKSPACE. */
int unetk_conv3d_pack_bf16(const float* w, int kd, int Cin, int Cout, void* wp_fwd, void* wp_dgrad, void* stream);
int unetk_conv3d_stat_rows_bf16(const unetk_conv3d_desc* d);
size_t unetk_conv3d_ws_bytes_bf16(const unetk_conv3d_desc* d);   /* 0 outside the rule */
int unetk_conv3d_fwd_bf16(const unetk_conv3d_desc* d, const float* x, const void* wp_fwd, float* y,
                          float* stat_partials, void* ws, size_t ws_bytes, void* stream);
int unetk_conv3d_dgrad_bf16(const unetk_conv3d_desc* d, const float* dy, const void* wp_dgrad, float* dx,
                            void* ws, size_t ws_bytes, void* stream);
int unetk_conv3d_wgrad_bf16(const unetk_conv3d_desc* d, const float* x, const float* dy, float* dw,
                            void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- normalisation + ReLU after each 3x3 conv
 * slim.batch_norm   NetworksV2/base.py:153-162 -- TF defaults eps 1e-3, decay .999 (GUNet encoder .99,
 *                   GUNet.py:321-325); training: batch mean + biased variance, unbiased variance into
 *                   the moving average; eval: moving statistics                        
 * slim.instance_norm base.py:163-165 -- eps 1e-6, moments over the spatial axes per (n, c)   (B4)
 * centre / scale are optional (gamma / beta may be NULL): GUNet.yml norm_with_center / norm_with_scale.
 * guide_ch > 0 adds GUNet's spatial modulation before the ReLU (GUNet.py:154-156,207-212):
 *   u += sum_g guide[n,pix,g] * gw[g][gw_coff + c] + gb[gw_coff + c]   (the 1x1 conv of the pooled guide,
 *   computed on the fly; gw is [guide_ch][gw_stride], gb is [gw_stride]). */
typedef struct unetk_norm_desc {
  int32_t N, HW, C;            /* activations [N, HW, C], dense */
  int32_t per_sample;          /* 0 = batch norm (one statistic group), 1 = instance norm (N groups) */
  int32_t z_stride;            /* pixel stride of the activated output (concat placement) */
  int32_t guide_ch, gw_stride, gw_coff;
  int32_t affine_only;         /* 1 = no normalisation (--without_norm, UNet.py:47-48: conv + bias + ReLU):
                                  backward skips the statistics terms, dbeta is the bias gradient */
  int32_t guide_leaky;         /* 3 = per-channel activation + post-shift on the guide branch (GUNet after_affine with --fix,
                                  GUNet.py:213-214,299-304): gb is a block of four rows of gw_stride floats -- bias, slope for
                                  s > 0, slope for s <= 0, post-shift -- and u = t * den + slope(s) * s + post-shift with
                                  s = guide . gw + bias; needs den; dgb comes back as the same block (slope rows zero);
                                  1 = LGNet's guide branch (LGNet.py:30-55): the 1x1 guide conv is followed by
                                  tf.nn.leaky_relu (alpha 0.2) before the add: u = t + lrelu(guide . gw + gb);
                                  needs guide_ch > 0, no density gains */
  int32_t storage;             /* UNETK_FP32: y / z / dz / dy are fp32; UNETK_BF16S: they are bf16 in memory (strides in
                                  elements), arithmetic, statistics and parameter gradients stay fp32 */
  float guide_alpha;           /* slope of the guide branch's activation when guide_leaky == 2 (guide_leaky == 1 is
                                  tf.nn.leaky_relu's default 0.2, LGNet): 0 = the ReLU of GUNet --fix (GUNet.py:299-304: the guide convs get norm + ReLU; the host
                                  folds that norm into gw / gb, exactly, from the guide's first and second moments) */
  float dropout_keep;          /* > 0: slim.dropout(keep_prob) on the NORMALISED value before the gains / guide term
                                  (GUNet --dropout, GUNet.py:189-190; training only); the 0 | 1/keep mask is regenerated
                                  from (dropout_seed, element index) in the forward and both backward passes.  With a guide
                                  or post-shift the backward needs the density variant (pass den = ones) */
  uint32_t dropout_seed;
  int32_t guide_per_sample;    /* 1: gw is [N][guide_ch][gw_stride], gb [N][gw_stride] (per-sample folded weights: --fix under
                                  instance norm) and dgw / dgb come back per sample; needs per_sample or den */
} unetk_norm_desc;

/* Finalise the conv's statistic partials ([2][stat_rows][C], each image's tiles contiguous) into
 * mean / rstd and the fused affine scale = gamma*rstd, shift = beta - mean*scale, each [groups][C].
 * Batch norm in training also updates the moving statistics; batch norm with training == 0 builds the
 * affine from the moving statistics and ignores the partials. */
size_t unetk_norm_finalize_ws_bytes(const unetk_norm_desc* d, int stat_rows);
int unetk_norm_finalize(const unetk_norm_desc* d, const float* stat_partials, int stat_rows,
                        const float* gamma, const float* beta, float eps, float decay, int training,
                        float* moving_mean, float* moving_var, float* mean_out, float* rstd_out,
                        float* scale_out, float* shift_out, void* ws, size_t ws_bytes, void* stream);
/* The same, given also the activations y [N, HW, C] the partials were taken of (fp32, dense, C % 4 == 0; NULL = exactly
 * unetk_norm_finalize).  A channel whose one-pass variance E[y^2] - E[y]^2 is ill-conditioned (mean^2 > 16 (var + eps))
 * gets its statistics recomputed on the device from y, shifted by the one-pass mean, in a fixed order; they replace the
 * one-pass ones where those are off by more than 2^-17 of rstd (2^-17 of the variance where the moving variance is
 * updated) or 2^-23 |mean| + 2^-21 std of the mean.  Every other channel's results are bit-identical to those of
 * unetk_norm_finalize.  Same workspace. */
int unetk_norm_finalize_y(const unetk_norm_desc* d, const float* stat_partials, int stat_rows, const float* y,
                          const float* gamma, const float* beta, float eps, float decay, int training,
                          float* moving_mean, float* moving_var, float* mean_out, float* rstd_out,
                          float* scale_out, float* shift_out, void* ws, size_t ws_bytes, void* stream);

/* z = relu((y*scale + shift) [* den[n][c]] [+ guide modulation]); z has pixel stride d->z_stride.
 * den (nullable, [N][C]) is GUNet's density modulation `conditional_normalization` (GUNet.py:119-133,203-206):
 * the per-sample channel gains the context MLP (unetk_fc_*) produced.  gb may be given with guide_ch == 0: a bare
 * per-channel shift after the gain -- with den = gain * gamma' this is `after_affine` (slim_nets.channel_wise_affine,
 * GUNet.py:213-214: (net) * gamma' + beta') in the same pass. */
int unetk_norm_apply_relu(const unetk_norm_desc* d, const void* y, const float* scale,
                          const float* shift, const float* den, const float* guide, const float* gw,
                          const float* gb, void* z, void* stream);

/* Backward of z = relu(norm(y) [* den] [+ modulation]).  Pass 1: per-group column sums of dt and dt*xhat
 * (du = dz * (z > 0), dt = du * den) [and du*guide_g, du, du*t]; pass 2: dy.  dz has pixel stride dz_stride.
 * Outputs (nullable when the parameter does not exist): dgamma[C], dbeta[C], dden[N][C] (required with den),
 * dgw[guide_ch][C], dgb[C]. */
size_t unetk_norm_bwd_ws_bytes(const unetk_norm_desc* d);
int unetk_norm_relu_bwd(const unetk_norm_desc* d, const void* y, const void* dz, int dz_stride,
                        const float* scale, const float* shift, const float* mean, const float* rstd,
                        const float* den, const float* guide, const float* gw, const float* gb, void* dy,
                        float* dgamma, float* dbeta, float* dden, float* dgw, float* dgb, void* ws,
                        size_t ws_bytes, void* stream);

/* unetk_norm_relu_bwd with the reduction pass already done by the kernel that produced dz (unetk_conv3x3_dgrad_nbr):
 * pre_partials [2][pre_rows][C], each statistics group's rows contiguous; NULL = unetk_norm_relu_bwd.  Plain units only
 * (no guide, density, dropout or bias-only mode: UNETK_E_UNSUPPORTED). */
int unetk_norm_relu_bwd_pre(const unetk_norm_desc* d, const void* y, const void* dz, int dz_stride,
                            const float* scale, const float* shift, const float* mean, const float* rstd,
                            const float* den, const float* guide, const float* gw, const float* gb, void* dy,
                            float* dgamma, float* dbeta, float* dden, float* dgw, float* dgb,
                            const float* pre_partials, int pre_rows, void* ws, size_t ws_bytes, void* stream);

/* unetk_norm_apply_relu of a plain unit (no guide / density / dropout) + unetk_maxpool2_fwd of its activation in ONE pass
 * (NetworksV2/UNet.py:79-80: slim.conv2d ... slim.max_pool2d): z as unetk_norm_apply_relu writes it (pixel stride
 * d->z_stride), pooled [N, H/2, W/2, C] dense.  d->HW = H * W, W given here, both even. */
int unetk_norm_apply_relu_pool(const unetk_norm_desc* d, int W, const void* y, const float* scale, const float* shift,
                               void* z, void* pooled, void* stream);

/* unetk_norm_relu_bwd for a plain unit (no guide / density / dropout) whose activation z feeds max_pool2d(2, 2) AND the skip
 * connection (NetworksV2/UNet.py:80-81,93: the second conv of every encoder level): replaces unetk_maxpool2_bwd (with its
 * `add` operand) + unetk_norm_relu_bwd -- the gradient of z, dskip + route(dp), is formed on the fly in both passes from
 * dskip (the skip's gradient: pixel stride dskip_stride, a channel slice of the concat buffer's gradient), dp (the pooled
 * tensor's gradient, [N, H/2, W/2, C] dense) and z re-evaluated from y; first maximum in window scan order takes dp
 * (TF MaxPoolGrad).  d->HW = H * W, W given here, both even.  Workspace: unetk_norm_bwd_ws_bytes(d). */
int unetk_norm_relu_bwd_pool(const unetk_norm_desc* d, int W, const void* y, const void* dskip, int dskip_stride,
                             const void* dp, const float* scale, const float* shift, const float* mean,
                             const float* rstd, void* dy, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                             void* stream);

/* GUNet --use_se (GUNet.py:192-201): the SE gate's input is pooled[b][c] = mean over the sample's pixels of the normalised
 * conv output, so the loss reaches y once more through it.  The norm backward is linear in dt, and this part of dt is the
 * per-(sample, channel) constant g[b][c] / HW: after unetk_norm_relu_bwd,  dy += scale * (A[b][c] - xhat * k2[group][c])
 * with A = g / HW - its mean over the statistics group and k2 = the group mean of (g / HW) * xhat (both [.][C], formed by
 * the caller from the per-sample means; zero under instance norm). */
int unetk_norm_se_bwd_add(const unetk_norm_desc* d, const void* y, void* dy, const float* mean,
                          const float* rstd, const float* scale, const float* A, const float* k2,
                          void* stream);

/* GUNet --use_se together with --dropout (NetworksV2/GUNet.py:189-201: the gate pools the DROPPED-OUT normalised output).
 * Forward: sums [2][N][C] = per (sample, channel) sum over the pixels of mask * xhat and of mask (xhat = (y - mean) rstd, the
 * 0 | 1/keep mask of d->dropout_keep / d->dropout_seed as the norm kernels regenerate it); pooled = gamma * sums[0] / HW +
 * beta * sums[1] / HW.  Backward: dy += scale * (mask * E[n][c] - k1 - xhat * k2) with E = d loss / d pooled / HW [N][C] and
 * k1, k2 [groups][C] the statistics group's means of mask E and mask E xhat (groups = N under instance norm, else 1). */
int unetk_norm_drop_pool(const unetk_norm_desc* d, const void* y, const float* mean, const float* rstd, float* sums, void* stream);
int unetk_norm_se_bwd_add_drop(const unetk_norm_desc* d, const void* y, void* dy, const float* mean, const float* rstd,
                               const float* scale, const float* E, const float* k1, const float* k2, void* stream);

/* ---------------------------------------------------------------- GUNet's context MLP (GUNet.py:136-150 `_context_subnets`)
 * slim.fully_connected(x, n): y[B][n] = act(x[B][k] . w[k][n] + b[n]), TF weight layout [in, out]; relu = 1 for the
 * hidden layers, 0 for the last (activation_fn=None), 2 = tf.nn.sigmoid (the SE gate of GUNet --use_se, GUNet.py:199).  slim.dropout(keep_prob) in training: mask from a counter
 * RNG keyed by (seed, element), kept entries scaled by 1/keep_prob; `mask` ([B][n] floats, 0 or 1/keep_prob,
 * nullable = no dropout) is written by the forward and read by the backward.
 * Backward: dx[B][k] (nullable), dw[k][n], db[n] from dy[B][n] (gated by y > 0 when relu, times the mask).
 * relu == 2 together with a mask returns UNETK_E_UNSUPPORTED from both calls before any launch: the backward sees only the
 * masked y = sigmoid(acc) * m, from which the derivative m * s * (1 - s) cannot be formed (no model drops out a gate). */
int unetk_fc_fwd(const float* x, const float* w, const float* b, float* y, float* mask, int B, int k, int n,
                 int relu, float keep_prob, uint32_t seed, void* stream);
int unetk_fc_bwd(const float* x, const float* w, const float* y, const float* mask, const float* dy, float* dx,
                 float* dw, float* db, float* dpre_ws, int B, int k, int n, int relu, void* stream);

/* ---------------------------------------------------------------- GUNet's 1-D VGG context models (slim_nets.py:60-144)
 * context_model "vgg16B" / "vgg16C" / "vgg16D" (GUNet.py:62-75; ext_config/GUNet_DE_VGG16{B,D}.yml): the context vector as
 * [B][L][1] through slim.conv1d (kernel k = 3 or 1, stride 1, SAME, bias, ReLU; w = TF [k][Cin][Cout]) and
 * tf.layers.max_pooling1d(2, 2, "same") (Lo = ceil(L / 2)); flattened [B][Lo * C] it feeds unetk_fc_*.
 * Backward: dx (nullable) / dw / db from dy gated by y > 0 when relu; dpre_ws = B * L * Cout floats of scratch.  The pool
 * backward routes to the first maximum of the window. */
int unetk_conv1d_fwd(const float* x, const float* w, const float* b, float* y, int B, int L, int Cin, int Cout, int k,
                     int relu, void* stream);
int unetk_conv1d_bwd(const float* x, const float* w, const float* y, const float* dy, float* dx, float* dw, float* db,
                     float* dpre_ws, int B, int L, int Cin, int Cout, int k, int relu, void* stream);
int unetk_maxpool1d_fwd(const float* x, float* y, int B, int L, int C, void* stream);
int unetk_maxpool1d_bwd(const float* x, const float* dy, float* dx, int B, int L, int C, void* stream);

/* tf.reduce_mean(x, axis=(1, 2)) of GUNet's conv context subnet (`_context_subnets_conv`, GUNet.py:83-116): x [N][HW][C] ->
 * y [N][C]; backward dx = dy / HW broadcast over the pixels. */
int unetk_spatial_mean_fwd(const float* x, float* y, int N, int64_t HW, int C, void* stream);
int unetk_spatial_mean_bwd(const float* dy, float* dx, int N, int64_t HW, int C, void* stream);

/* ---------------------------------------------------------------- slim.max_pool2d(x, [2,2])  UNet.py:81
 * VALID, stride 2.  x [N,H,W,C] with pixel stride x_stride; p dense [N,H/2,W/2,C].
 * Backward routes dp to the first maximum in window scan order (TF MaxPoolGrad); `add` (nullable, [N,H,W,C] with
 * pixel stride add_stride) is summed into dx: x's other consumer is the skip connection (UNet.py:93), whose gradient
 * is the first half of the concat buffer's gradient -- one pass instead of a pool backward plus an add. */
int unetk_maxpool2_fwd(const float* x, int x_stride, float* p, int N, int H, int W, int C,
                       void* stream);
int unetk_maxpool2_bwd(const float* x, int x_stride, const float* p, const float* dp, const float* add,
                       int add_stride, float* dx, int N, int H, int W, int C, void* stream);
/* UNETK_BF16S variants: x, p, dp, add, dx are bf16 (strides in elements); the skip gradient is summed in fp32 and
 * rounded once. */
int unetk_maxpool2_fwd_bf16(const void* x, int x_stride, void* p, int N, int H, int W, int C, void* stream);
int unetk_maxpool2_bwd_bf16(const void* x, int x_stride, const void* p, const void* dp, const void* add,
                            int add_stride, void* dx, int N, int H, int W, int C, void* stream);
/* slim.avg_pool2d(gs, 2) of GUNet's spatial-guide pyramid (GUNet.py:157-158); x, p dense, any C. */
int unetk_avgpool2_fwd(const float* x, float* p, int N, int H, int W, int C, void* stream);
/* Moments of the (pooled) spatial guide [N, HW, G] per statistics group (1 group, or N with per_sample):
 * out[grp][0..G) = E[g_i], out[grp][G + i G + j] = E[g_i g_j].  GUNet --fix normalises the guide's 1x1 conv
 * (GUNet.py:299-304); that conv being linear in the guide, its statistics follow exactly from these numbers. */
int unetk_guide_moments(const float* guide, int N, int64_t HW, int G, int per_sample, float* out, void* stream);
/* --img_grad (UNet.py:69-71, GUNet.py:335-338): out [N,H,W,3C] = concat(x, dy, dx) with
 * tf.image.image_gradients' forward differences (dy[h] = x[h+1] - x[h], last row 0; dx likewise). */
/* InterUNet's --img_grad input (InterUNet.py:105-109): out [N,H,W,C+2] = concat(x, sobel_dy(x[..., ch]), sobel_dx(x[..., ch]))
 * with tf.image.sobel_edges' kernels over the REFLECT-padded channel. */
int unetk_sobel_concat(const float* x, float* out, int N, int H, int W, int C, int ch, void* stream);
int unetk_image_gradients(const float* x, float* out, int N, int H, int W, int C, void* stream);
/* Mirror test-time augmentation (evaluators/evaluator_liver.py:648-655; the reference flips on the host with
 * np.flip): out[n,h,w,:] (+)= scale * x[n, flip_h ? H-1-h : h, flip_w ? W-1-w : w, :].  x != out. */
int unetk_flip_axpy(const float* x, float* out, int N, int H, int W, int C, int flip_h, int flip_w,
                    float scale, int accumulate, void* stream);

/* ---------------------------------------------------------------- slim.conv2d_transpose(x, C, 2, 2)
 * UNet.py:91-93: kernel 2 stride 2, bias, ReLU, then tf.concat((skip, up), -1).
 * out[n,2y+a,2x+b, out_coff+co] = relu(sum_ci x[n,y,x,ci]*w[a,b,co,ci] + bias[co]),
 * written straight into the concat buffer (pixel stride out_stride). */
typedef struct unetk_deconv_desc {
  int32_t N, H, W, Cin, Cout; /* input geometry; output is [N,2H,2W,Cout] */
  int32_t out_stride, out_coff;
  int32_t precision; /* UNETK_FP32 / UNETK_BF16 (Cin % 32 == 0 and Cout % 32 == 0; filters from *_pack_bf16) /
                        UNETK_BF16S (x, out / cat, dcat, dx are bf16; Cin % 64 == 0 and Cout % 32 == 0) */
} unetk_deconv_desc;

/* wp_fwd: [Cin/4][4*Cout][4]; wp_dgrad: [4*Cout/4][Cin][4]; each 4*Cin*Cout floats. */
int unetk_deconv2x2_pack(const float* w, int Cin, int Cout, float* wp_fwd, float* wp_dgrad,
                         void* stream);
/* UNETK_BF16: wp_fwd [Cin/8][4*Cout][8], wp_dgrad [4*Cout/8][Cin][8], each 4*Cin*Cout bf16. */
int unetk_deconv2x2_pack_bf16(const float* w, int Cin, int Cout, void* wp_fwd, void* wp_dgrad,
                              void* stream);
/* UNETK_BF16S: the bf16 packs with the GEMM columns permuted inside every 64-column block (see
 * unetk_conv3x3_pack_bf16s).  Cin % 64 == 0 and Cout % 64 == 0. */
int unetk_deconv2x2_pack_bf16s(const float* w, int Cin, int Cout, void* wp_fwd, void* wp_dgrad,
                               void* stream);
int unetk_deconv2x2_fwd(const unetk_deconv_desc* d, const void* x, const void* wp_fwd,
                        const float* bias, void* out, void* stream);
/* Backward.  dcat/cat: gradient and forward value of the concat buffer (same strides/offset as
 * `out`).  Produces dx [N,H,W,Cin], dw [2,2,Cout,Cin], dbias [Cout].  Needs Cin % 64 == 0, Cout % 32 == 0 (UNETK_BF16S:
 * % 64), Cout <= 1024, out_stride % 4 == 0 and out_coff % 4 == 0; otherwise UNETK_E_UNSUPPORTED and a zero *_ws_bytes. */
size_t unetk_deconv2x2_bwd_ws_bytes(const unetk_deconv_desc* d);
int unetk_deconv2x2_bwd(const unetk_deconv_desc* d, const void* x, const void* wp_dgrad,
                        const void* cat, const void* dcat, void* dx, float* dw, float* dbias,
                        void* ws, size_t ws_bytes, void* stream);

/* slim.conv3d_transpose(x, c, kernel == stride in {(1,2,2), (2,2,2)}, biases_initializer=None) + tf.concat,
 * NetworksV2/UNet3D.py:161-163.  x [N,D,H,W,Cin]; out [N,kd*D,2H,2W,...]; filter TF [kd,2,2,Cout,Cin];
 * bias / dbias may be NULL (UNet3D has none).  The 2-D functions above are the D = 1, kd = 1 case. */
typedef struct unetk_deconv3d_desc {
  int32_t N, D, H, W, Cin, Cout;
  int32_t kd; /* depth kernel == depth stride: 1 or 2 */
  int32_t out_stride, out_coff;
  int32_t precision; /* UNETK_FP32 / UNETK_BF16 / UNETK_BF16S (as unetk_deconv_desc) */
} unetk_deconv3d_desc;
int unetk_deconv3d_pack(const float* w, int kd, int Cin, int Cout, float* wp_fwd, float* wp_dgrad,
                        void* stream);
int unetk_deconv3d_pack_bf16(const float* w, int kd, int Cin, int Cout, void* wp_fwd, void* wp_dgrad,
                             void* stream);
int unetk_deconv3d_fwd(const unetk_deconv3d_desc* d, const void* x, const void* wp_fwd,
                       const float* bias, void* out, void* stream);
size_t unetk_deconv3d_bwd_ws_bytes(const unetk_deconv3d_desc* d);
int unetk_deconv3d_bwd(const unetk_deconv3d_desc* d, const void* x, const void* wp_dgrad,
                       const void* cat, const void* dcat, void* dx, float* dw, float* dbias,
                       void* ws, size_t ws_bytes, void* stream);
/* The same in two parts (ABI 9): parts bit 0 = ReLU backward + dbias + dx (leaves the masked, re-laid gradient in ws), bit 1 = dw
 * (reads it from the SAME ws; any stream ordered behind the bit-0 call).  The filter gradient is off the critical chain of the
 * backward pass (TF schedules Conv2DBackpropFilter beside the rest of the graph the same way); parts = 3 is unetk_deconv3d_bwd. */
int unetk_deconv3d_bwd_parts(const unetk_deconv3d_desc* d, const void* x, const void* wp_dgrad,
                             const void* cat, const void* dcat, void* dx, float* dw, float* dbias,
                             void* ws, size_t ws_bytes, int parts, void* stream);
int unetk_deconv2x2_bwd_parts(const unetk_deconv_desc* d, const void* x, const void* wp_dgrad,
                              const void* cat, const void* dcat, void* dx, float* dw, float* dbias,
                              void* ws, size_t ws_bytes, int parts, void* stream);

/* ---------------------------------------------------------------- logits + loss head
 * UNet.py:97-135 + loss_metrics.py:115-231,261-339.
 * logits = z @ w[C,ncls] + b  (slim.conv2d(x, ncls, 1), linear);  softmax;  weighted sparse
 * softmax cross-entropy with SUM_BY_NONZERO_WEIGHTS and/or soft Dice loss;  thresholded
 * (prob > 0.5) per-class counts for metric_dice / metric_voe / metric_vd. */
typedef struct unetk_head_desc {
  int32_t N, HW, C, ncls;
  int32_t weight_mode;                    /* UNETK_W_* */
  float numeric_w[UNETK_MAX_CLASSES];     /* --loss_numeric_w */
  float proportion_decay;                 /* --loss_proportion_decay (<=0: none) */
  int32_t storage;                        /* UNETK_FP32, or UNETK_BF16S: the feature map z and its gradient dz are bf16
                                             (logits, probabilities, losses and dw / db stay fp32) */
} unetk_head_desc;

/* Reduced outputs of the forward pass (device, floats), layout:
 *   [0] xent loss  [1] dice loss  [2] num_present
 *   then per sample b, per foreground class c=1..ncls-1 (index 3 + (b*(ncls-1)+(c-1))*4 + k):
 *     k=0 sum(pred*lab) k=1 sum(pred) k=2 sum(lab) k=3 sum(clip(pred+lab,0,1))
 *   then per sample b: I_b, U_b  (soft dice intersection / union, loss_metrics.py:217-218) */
size_t unetk_head_result_floats(const unetk_head_desc* d);
size_t unetk_head_ws_bytes(const unetk_head_desc* d);
/* logits [N*HW, ncls] always written; probs (same shape) optional; pixel_w only for PIXELMAP. */
int unetk_head_fwd(const unetk_head_desc* d, const void* z, const float* w, const float* b,
                   const int32_t* labels, const float* pixel_w, float* logits, float* probs,
                   float* result, void* ws, size_t ws_bytes, void* stream);
/* Backward of (xent_scale * xent + dice_scale * dice) w.r.t. z, w, b.  `result` and `ws` are
 * the buffers the forward filled (ws keeps the per-sample weight tables).  dev_scales (nullable)
 * points at two device floats multiplied into xent_scale / dice_scale (upstream gradients that
 * live on the device -- avoids a host sync). */
int unetk_head_bwd(const unetk_head_desc* d, const void* z, const float* w,
                   const int32_t* labels, const float* pixel_w, const float* logits,
                   const float* result, float xent_scale, float dice_scale,
                   const float* dev_scales, void* dz, float* dw, float* db, void* ws,
                   size_t ws_bytes, void* stream);
/* Inference helpers: evaluators/evaluator_liver.py:663 np.argmax(prob, -1) (lowest index on ties)
 * and UNet.py:112-118 Pred_c = prob_c > 0.5 (uint8).  preds is [ncls-1][npix] or NULL. */
int unetk_head_predict(const float* probs, int64_t npix, int ncls, uint8_t* argmax,
                       uint8_t* preds, void* stream);

/* --loss_weight_type boundary (loss_metrics.py:149-165; 2-D only, as in the reference): labels int32
 * [N,H,W] -> wmap f32 [N,H,W] = normalised exp(-EDT/25) + 1, EDT = exact Euclidean distance to the nearest
 * pixel of the 3x3 dilation ring of any class (the reference round-trips to scipy on the host through
 * tf.py_func; this runs on the device).  Feed wmap to unetk_head_fwd/bwd as UNETK_W_PIXELMAP. */
size_t unetk_boundary_weights_ws_bytes(int N, int H, int W);
int unetk_boundary_weights(const int32_t* labels, int N, int H, int W, float* wmap, void* ws,
                           size_t ws_bytes, void* stream);

/* --loss_weight_type boundary for UNet3D (a project extension: the reference's _compute_weights reshapes a 4-D
 * one-hot tensor and fails on 5-D).  For labels int32 [N, D, H, W], an integer z scale K >= 1 (the slice spacing in units of the
 * in-plane spacing), and each sample on its own:
 *   ring(z,y,x)  some in-bounds voxel of the 3x3x3 neighbourhood carries a label different from the voxel's own.  This equals
 *                sum_c (clip(conv3d(onehot_c, ones(3,3,3), SAME), 0, 1) - onehot_c) > 0, the 3-D form of the reference's 2-D ring.
 *   d2(z,y,x)  = min over ring voxels (K (z - z'))^2 + (y - y')^2 + (x - x')^2.  This is an exact integer.
 *   d          = (float) sqrt((double) d2).  This is bit for bit what
 *                scipy.ndimage.distance_transform_edt(~ring, sampling=(K,1,1)).astype(float32) returns.
 *   w          = expf(-d / 25) + 1, then w * (D H W) / sum(w) per sample.  The sum is taken in a fixed order, so two runs give
 *                identical bits.
 * A sample without any ring voxel (a single-label patch) gets w = 1 everywhere and d2 = -1.  This is a rule of this project:
 * scipy's answer for an input without zeros is an artefact, and the 2-D entry's reproduction of that artefact is not carried
 * into 3-D.
 * wmap f32 [N, D, H, W] feeds unetk_head_fwd/bwd as UNETK_W_PIXELMAP with HW = D H W; it also serves as scratch during the call.
 * d2_out int32 [N, D, H, W] is nullable: when it is null, nothing extra is written.
 * Limits: 1 <= z_scale <= 16, D <= 1024, H, W <= 4096 and N D H ceil(W / 64) < 2^31, else UNETK_E_UNSUPPORTED (under these caps
 * d2 < 2^31, and no intermediate overflows int32); N <= 65535 and 4-byte aligned labels / wmap / d2_out, else UNETK_E_BADARG.
 * Workspace (16-byte aligned, else UNETK_E_BADARG; short: UNETK_E_WORKSPACE; the query returns 0 for extents the entry refuses):
 *   8 * N * H * ceil(W / 64) * ceil(D / 16)   one double per block of the z pass, the sums of the weights
 * + 4 * N * D * H * W                         the int32 field between the y and the z pass */
size_t unetk_boundary_weights3d_ws_bytes(int N, int D, int H, int W);
int unetk_boundary_weights3d(const int32_t* labels, int N, int D, int H, int W, int z_scale, float* wmap,
                             int32_t* d2_out /* nullable, [N,D,H,W] */, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- volume evaluation
 * evaluators/evaluator_liver.py:680-702,906-996 (_postprocess, _run_actual) and loss_metrics.py:342-452 (metric_3d), which
 * the reference runs on the host with scipy.  Masks are dense C-order uint8 [D,H,W], non-zero = object.  D, H, W > 0
 * (else UNETK_E_BADARG) and D*H*W < 2^31 (else UNETK_E_UNSUPPORTED; the *_ws_bytes queries then return 0).  Workspaces are
 * 16-byte aligned, of at least the queried size; every reduction runs in a fixed order, so results are bit-reproducible.
 *
 * unetk_largest_component: out = the largest 6-connected component of mask (0/1), the one with the larger root (minimum
 *   linear index of the component) on ties -- utils/array_kits.py:357-384 get_largest_component(x, rank=3), whose scipy
 *   labels number components in raster order of their roots and whose tie rule is "the last of np.argsort(areas)".  An
 *   empty mask gives zeros.  Union-find with integer atomicMin (each voxel ends at the minimum index of its component),
 *   sizes by integer atomics, one packed 64-bit (size, root) max.  info int32[4] = {root (-1 if empty), its size, number
 *   of components of that size, number of components}.  The workspace then holds the component table: int32 label[n] at
 *   offset 0 (the root of each voxel, -1 = background) and int32 size[n] at offset (4n + 255) & ~255 (each component's
 *   size at its root, 0 elsewhere), n = D*H*W.  np.argsort is stable only for short arrays, so when info[2] > 1 a caller
 *   that must match the host exactly runs the host's argsort over the sizes in root order and passes its pick to
 *   unetk_component_mask, which rewrites out = (label == root) from that table.
 * unetk_mask_counts: counts int64[4] = {|A|, |B|, |A and B|, |A or B|} (tp = [2], fp = [0] - [2], fn = [1] - [2]).
 * unetk_surface3d: edge = A xor erode(A, 18-neighbourhood), the volume border counting as background (utils/surface.py
 *   Surface.compute_contour).  box int32[6] = {z0, y0, x0, z1, y1, x1} (half-open) receives the bounding box of the edge
 *   voxels: reset first unless accumulate_box (then widened: two calls give the union box of two surfaces); it stays empty
 *   (z1 = 0) for an empty edge.
 * unetk_edt3d_sq: dist2 f64 [D,H,W] = squared Euclidean distance, with voxel spacing (sz, sy, sx) > 0, from each voxel
 *   inside the device box to the nearest non-zero voxel of `feature` -- scipy.ndimage.distance_transform_edt(~feature,
 *   sampling)^2.  Exact when the box holds every feature voxel; voxels outside the box are not written.  Three separable
 *   1-D passes (lower envelope of parabolas), one line per thread.
 * unetk_surface_dist: over the non-zero voxels of surf, d = sqrt(dist2): out = {sum d, sum d^2, max d} as f64 and the
 *   count as int64 in the fourth 8-byte slot; zeros for an empty surf.  ASSD / RMSD / MSD follow on the host. */
size_t unetk_largest_component_ws_bytes(int D, int H, int W);
int unetk_largest_component(const uint8_t* mask, int D, int H, int W, uint8_t* out, int32_t* info, void* ws,
                            size_t ws_bytes, void* stream);
int unetk_component_mask(const void* ws, int D, int H, int W, int32_t root, uint8_t* out, void* stream);
/* unetk_fp_mask3d (additive to ABI 10): the false-positive objects of a saved prediction, mined for
 *   hard-negative training -- DataLoader/NF/input_pipeline_3d.py:187-219 load_neg.  pred, lab, out uint8 [D,H,W]; lab in the
 *   store's encoding.  Predicted object: pred >= pred_label; labelled object: lab / lab_scale >= obj_label.  The components of
 *   the predicted object are 6-connected (the union-find of unetk_largest_component).  A component is KEPT when it holds at
 *   least min_size voxels and shares no voxel with the labelled object (the reference drops sizes <= 5: min_size 6; it tests
 *   the overlap against any non-zero label, its labels being binary).  out = out_value on kept components, 0 elsewhere (every
 *   voxel is written; out may be pred itself); slice_counts int32 [D] = kept voxels per slice; head int32 [4] = {components,
 *   kept components, kept voxels, 0}.  Integer arithmetic and integer atomics only, whose order cannot change a result: two
 *   calls give identical bits.  pred_label, lab_scale, obj_label, min_size >= 1, 1 <= out_value <= 255 (else UNETK_E_BADARG).
 *   ws (16-byte aligned): int32 label[n], then int32 size[n] at offset (4n + 255) & ~255. */
size_t unetk_fp_mask3d_ws_bytes(int D, int H, int W);
int unetk_fp_mask3d(const uint8_t* pred, const uint8_t* lab, int D, int H, int W, int pred_label, int lab_scale, int obj_label,
                    int min_size, int out_value, uint8_t* out, int32_t* slice_counts, int32_t* head, void* ws, size_t ws_bytes,
                    void* stream);
size_t unetk_mask_counts_ws_bytes(int D, int H, int W);
int unetk_mask_counts(const uint8_t* a, const uint8_t* b, int D, int H, int W, int64_t* counts, void* ws,
                      size_t ws_bytes, void* stream);
int unetk_surface3d(const uint8_t* mask, int D, int H, int W, uint8_t* edge, int32_t* box, int accumulate_box,
                    void* stream);
size_t unetk_edt3d_sq_ws_bytes(int D, int H, int W);
int unetk_edt3d_sq(const uint8_t* feature, int D, int H, int W, const int32_t* box, double sz, double sy, double sx,
                   double* dist2, void* ws, size_t ws_bytes, void* stream);
size_t unetk_surface_dist_ws_bytes(int D, int H, int W);
int unetk_surface_dist(const uint8_t* surf, const double* dist2, int D, int H, int W, double* out, void* ws,
                       size_t ws_bytes, void* stream);
/* Per-slice HU histograms of a case, the context guide's feature rows (DataLoader/Liver/extract.py:237-375,
 * dump_hist_feature / dump_hist_feature_v2).  vol int16 [D,H,W] HU, lab uint8 [D,H,W]; out f32 [D, 2 bins]:
 *   columns [0, bins): the values of slice k where lab >= 1;
 *   columns [bins, 2 bins): mode 0 (train) the values of slice k where lab == 2; mode 1 (eval) the values of every
 *   18-connected tumour component c (lab == 2) whose z-extent [z0, z1) covers k, taken on c's middle slice
 *   m = (z1 - z0 - 1) / 2 + z0 (array_kits.guide_pixel_list(middle, tile_guide)).
 * Bins through the host's table: value v counts in bin lut[v - lut_lo] when 0 <= v - lut_lo < lut_n and that entry is >= 0
 * (the host applies np.histogram's edge rule); each half-row is np.histogram(density=True) = (count / db[b]) / total in
 * fp64 with db f64 [bins] the bin widths, rounded to f32, and 0 when the half is empty.  Counts are integer atomics, so the
 * rows are bit-reproducible.  bins <= 1024; ws 16-byte aligned, at least unetk_slice_hist_ws_bytes (mode 1 holds two int32
 * per voxel for the union-find). */
size_t unetk_slice_hist_ws_bytes(int D, int H, int W, int bins, int mode);
int unetk_slice_hist(const int16_t* vol, const uint8_t* lab, int D, int H, int W, int mode, const int32_t* lut, int lut_lo,
                     int lut_n, const double* db, int bins, float* out, void* ws, size_t ws_bytes, void* stream);
/* Grey-level co-occurrence texture features of uint8 patches, the `glcm` context rows (DataLoader/Liver/extract.py:377-661 ->
 * utils/array_kits.py:1140-1232 glcm_features / greycoprops on skimage's greycomatrix(levels=256, symmetric, normed)).
 * pix: device bytes; patch p is the row-major h x w uint8 image at pix + patch_tab[p][0] (any byte alignment).  patch_tab int32
 * [n][3] = (byte offset, h, w) and offsets int32 [K][2] = (dr, dc) are HOST arrays: they are checked before anything is
 * launched and the table is copied into the workspace on `stream`.  For patch p and offset k every pixel (r, c) whose partner
 * (r + dr, c + dc) lies inside the patch counts once at [img[r, c]][img[r + dr, c + dc]]; S = C + C^T, P = S / sum(S) (sum
 * taken as 1 when there is no pair, so P = 0).  out f64 [n][8][K], property order contrast, dissimilarity, homogeneity, energy,
 * entropy (-sum P log(P + 1e-16)), correlation (exactly 1 when a standard deviation is below 1e-15; centred two-pass form),
 * cluster_shade, cluster_prominence; norm_levels != 0 applies glcm_features' scaling for 256 levels (contrast / 4096,
 * dissimilarity / 64, homogeneity x 2, energy x 2, entropy / 8, shade / 64^3, prominence / 64^4).  counts_out (nullable) u32
 * [n][K][256][256] receives S.  Counts are integer LDS atomics and the fp64 sums run in a fixed order: bit-reproducible.
 * One workgroup per (p, k) with S's upper triangle in 131,584 B of LDS.
 * UNETK_E_UNSUPPORTED (and a workspace query of 0): n < 1, K < 1, K > 16, n > 2^24; also h or w outside [1, 4096] and
 * pix_bytes >= 2^31.  UNETK_E_BADARG: null pix / patch_tab / offsets / out / ws, patch_tab or offsets or counts_out not 4-byte,
 * out not 8-byte, ws not 16-byte aligned, a patch reaching past pix_bytes.  UNETK_E_WORKSPACE: ws_bytes below the query. */
size_t unetk_glcm_features_ws_bytes(int n, int K);
int unetk_glcm_features(const uint8_t* pix, int64_t pix_bytes, const int32_t* patch_tab, int n, const int32_t* offsets, int K,
                        int norm_levels, double* out, uint32_t* counts_out, void* ws, size_t ws_bytes, void* stream);

/* Spatial-guide propagation of the guided volume evaluation (DataLoader/Liver/input_pipeline_g.py:1179-1513,
 * EvalImage3DLoader), one slice at a time; the matching itself stays on the host.
 * unetk_guide_components: acc f32 [H,W,3] the slice's mirror-averaged class probabilities, guide f32 [H,W] the guide the
 *   slice was given.  Tumour mask = argmax(acc) == 2 (lowest index on ties); its 4-connected components (the labels of
 *   unetk_largest_component with D = 1, numbered in increasing root = minimum linear index, scipy's order).  table int32
 *   [4 + cap * 12]: head {count, overflow (count > cap), 0, 0}, then per component k < min(count, cap) the row
 *   {root, area, y0, x0, y1, x1 (inclusive box), peak index, peak value (f32 bits), cy, cx, sy, sx (f32 bits)}: the peak
 *   is the maximum of guide over the component at its first raster position, (cy, cx) the medians of its rows and columns
 *   (mean of the two middle values for even counts) and (sy, sx) = 1.4826f * the median absolute deviations in float32 --
 *   array_kits.compute_robust_moments without the min_std floor.  Exact: integer histograms, then one thread per component.
 *   H * W < 2^31, 0 < cap <= 65536, cap * H < 2^31 and cap * W < 2^31 (else UNETK_E_BADARG and a zero ws query);
 *   ws 16-byte aligned, at least unetk_guide_components_ws_bytes.
 * unetk_guide_render: guide f32 [H,W] = max_k exp(-((y - cy)^2 / (2 sy^2) + (x - cx)^2 / (2 sx^2))) * discount / 2 + 0.5
 *   over obj float4 [n_obj] = (cy, cx, sy, sx), 16-byte aligned (array_kits.create_gaussian_distribution_v2 in float32);
 *   exactly 0.5 when n_obj = 0. */
size_t unetk_guide_components_ws_bytes(int H, int W, int cap);
int unetk_guide_components(const float* acc, const float* guide, int H, int W, int cap, int32_t* table, void* ws,
                           size_t ws_bytes, void* stream);
int unetk_guide_render(const float* obj, int n_obj, int H, int W, float discount, float* guide, void* stream);

/* Per-lesion detection (additive to ABI 10): the component tables that utils/array_kits.py:883-984
 * distinct_binary_object_correspondences builds with scipy.ndimage.label and np.unique; the matching rule itself stays on
 * the host (utils/array_kits.match_components).  res, ref uint8 [D,H,W], non-zero = object.  Both masks are labelled by the
 * union-find of unetk_largest_component (6-connected, every voxel ends at the minimum linear index of its component) and
 * their components numbered 1..n in increasing root: scipy.ndimage.label's ids with generate_binary_structure(3, 1).
 * table int32 [4 + 4 cap_obj + 3 cap_pair]:
 *   head {n_res, n_ref, n_pair, overflow}: the true counts whatever the caps; overflow bit 0 = n_res > cap_obj,
 *     bit 1 = n_ref > cap_obj, bit 2 = n_pair > cap_pair;
 *   cap_obj rows {root, size} of res, then cap_obj rows {root, size} of ref, row k = the component of id k + 1;
 *   cap_pair rows {ref_id, res_id, overlap}: one for every pair of components that share a voxel, sorted by
 *     (ref_id, res_id).  The pair rows are written only when no overflow bit is set.
 * Rows past the counts are zero.  Integer arithmetic throughout; the pairs are ranked before their rows are written, so the
 * table is the same bit for bit from run to run.  0 < cap_obj, cap_pair <= 2^24 (else UNETK_E_BADARG and a zero ws query);
 * table 4-byte, ws 16-byte aligned, at least unetk_component_overlaps_ws_bytes (16 bytes per voxel and 16 per pair row). */
size_t unetk_component_overlaps_ws_bytes(int D, int H, int W, int cap_obj, int cap_pair);
int unetk_component_overlaps(const uint8_t* res, const uint8_t* ref, int D, int H, int W, int cap_obj, int cap_pair,
                             int32_t* table, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- offline evaluation: slabs in, zoom back
 * The input and the output side of evaluators/evaluator_liver.py on the device (csrc/evalio.hip); both are gathers that
 * write every output element once: no atomics, no workspace.
 *
 * Slab building (DataLoader/Liver/input_pipeline.py:556-668, input_pipeline_li.py:398-456): images f32 [N,H,W,C] dense =
 * window-normalised, bilinearly resized planes of the resident raw crop vol int16 [src_d,src_h,src_w].  zsrc int32 [N,C]:
 * the plane of every sample and channel: >= 0 a slice of vol, -1 a plane of exactly 0.0f, -2 a plane of HU 0 passed
 * through the window (context padded before normalisation).  Window: HU is clamped into [lo, hi] and read from
 * lut f32 [lut_n >= hi - lo + 1], lut[v - lo] = the host's normalisation of v (-32768 <= lo <= hi <= 32767, at most
 * 16384 entries).  Resize: the host's six tap arrays y0, y1 int32 [H], fy f32 [H], x0, x1 int32 [W], fx f32 [W] (taps
 * are clamped into the plane); rows first, r = a[y0] * (1 - fy) + a[y1] * fy, then columns r[x0] * (1 - fx) + r[x1] * fx,
 * every product, sum and difference rounded to f32 on its own (no FMA): bit-equal to numpy's float32 arithmetic.
 * src_d * src_h * src_w < 2^31 and N * H * W * C < 2^31; images 4-byte aligned (16-byte aligned: 16-byte stores). */
int unetk_eval_slab(const int16_t* vol, int src_d, int src_h, int src_w, const int32_t* zsrc, int N, int C,
                    const int32_t* y0, const int32_t* y1, const float* fy, int H, const int32_t* x0, const int32_t* x1,
                    const float* fx, int W, const float* lut, int lut_n, int lo, int hi, float* images, void* stream);
/* Zoom back (evaluator_liver.py:670-676, scipy.ndimage.zoom with order 0, separable): dst uint8 [D,H,W] dense,
 * dst[z][y][x] = src[tz[z]][ty[y]][tx[x]] with src uint8 [d,h,w], tz int32 [D], ty int32 [H], tx int32 [W]; an index of
 * -1 (any index outside its axis) writes 0: scipy's samples that land just outside the input.  d * h * w < 2^31 and
 * D * H * W < 2^31. */
int unetk_zoom_nearest3d(const uint8_t* src, int d, int h, int w, const int32_t* tz, const int32_t* ty, const int32_t* tx,
                         int D, int H, int W, uint8_t* dst, void* stream);
/* Saved prediction (evaluator_liver.py:998-1026 `maybe_save_case`, nii_kits.py:53-75 `write_nii`): the post-processed class
 * masks of one case -- liver and / or tumor, uint8 [bd,bh,bw] in (z, y, x) order, either may be NULL -- placed at
 * (z1, y1, x1) of a [d,h,w] volume of zeros and written as int16 in NIfTI file order: dst[i0 + n0 * (i1 + n1 * i2)] with
 * file axis k running along data axis t_k (0 = z, 1 = y, 2 = x; n_k its length; (t0, t1, t2) a permutation: write_nii's
 * `trans_bk`), backwards along the data axes whose bit of `flips` is set (bit 0 = x, 1 = y, 2 = z).  The value is
 * liver + tumor inside the box and 0 outside; every one of the d * h * w elements is written exactly once; no workspace.
 * t0 == 2 (every LiTS file): 16-byte stores, 8-byte mask reads (dst not 16-byte aligned: one element per thread);
 * otherwise a tiled transpose through LDS.  UNETK_E_BADARG: dst or both masks NULL, dst not 2-byte aligned, a
 * non-positive size, a box outside the case, (t0, t1, t2) not a permutation; UNETK_E_UNSUPPORTED: d * h * w >= 2^31. */
int unetk_nii_compose(const uint8_t* liver, const uint8_t* tumor, int bd, int bh, int bw, int z1, int y1, int x1, int d, int h,
                      int w, int t0, int t1, int t2, int flips, int16_t* dst, void* stream);
/* A NIfTI volume into store slices (nii_kits.py:33-50 `read_nii` and DataLoader/Liver/extract.py:72): the
 * inverse walk of unetk_nii_compose.  src: the file's voxel block as it lies in the file behind vox_offset (little-endian), on
 * the device, n0 * n1 * n2 elements of NIfTI `datatype` (2 uint8, 4 int16, 8 int32, 16 float32, 64 float64, 256 int8,
 * 512 uint16, 768 uint32), file axis 0 fastest.  (t0, t1, t2) and `flips` in unetk_nii_compose's convention: file axis k runs
 * along data axis t_k (0 = z, 1 = y, 2 = x), backwards along the data axes whose bit of `flips` is set (bit 0 = x, 1 = y,
 * 2 = z).  dst uint16 [d,h,w] dense in (z, y, x) order (the int16-typed storage of a slice store), d, h, w = the n_k of the
 * file axes along z, y, x; every element is written exactly once by plain stores; no workspace.
 * Value, bit for bit the host's: v = (double)raw, and v * scl_slope + scl_inter (product and sum rounded on their own) when
 * scl_slope is neither 0 nor NaN; v16 = v cast to int16 by truncation toward zero -- where numpy leaves the cast undefined this
 * library defines it: NaN gives 0, values beyond [-32768, 32767] saturate; dst = (min(max(v16, lo), hi) - lo) * scale.  The
 * store's encoding is lo = -250, hi = 300, scale = 64 (extract.py:32-35).
 * t0 == 2 (every LiTS file): int16 without scaling from a 16-byte aligned src moves in 16-byte loads and, where the row's place
 * in dst is 16-byte aligned, 16-byte stores, reversed in the registers under an x flip; any other datatype, a scaled source or
 * a src that is not 16-byte aligned goes one element per thread.  t0 != 2: a tiled transpose through LDS, reads and writes
 * both coalesced.  UNETK_E_BADARG (nothing is written): src or dst NULL, dst not 2-byte aligned, src not aligned for its
 * datatype, an unknown datatype, a non-positive size or scale, (t0, t1, t2) not a permutation, flips outside 0..7, lo > hi,
 * (hi - lo) * scale > 65535; UNETK_E_UNSUPPORTED: n0 * n1 * n2 >= 2^31. */
int unetk_nii_ingest(const void* src, int datatype, int n0, int n1, int n2, double scl_slope, double scl_inter, int t0, int t1,
                     int t2, int flips, int lo, int hi, int scale, uint16_t* dst, void* stream);

/* ---------------------------------------------------------------- LiTS training batch  
 * DataLoader/Liver/input_pipeline.py:243-284 `data_processing_train` for a whole batch, gathering from decoded slices
 * that are RESIDENT in device memory: per sample crop_to_bounding_box -> resize_bilinear(align_corners) -> window clip
 * -> normalise (images), crop -> resize_nearest_neighbor(align_corners) -> / lab_scale (labels), uniform noise
 * U(-noise_scale, noise_scale) on non-padding slices (counter-based generator keyed by `seed`), random flips.
 * slices: uint16 [n_slices, src_h, src_w]; seg_slices: uint8 [n_slices, src_h, src_w];
 * sample_tab int32 [N][C + 7] = {slice index x C (-1 = zero padding), label slice index (-1 = zeros), off_y, off_x,
 * crop_h, crop_w, flip_left_right, flip_up_down}; clip float [N][2] = {lo, hi};
 * images f32 [N,H,W,C]; labels int32 [N,H,W].  The caller guarantees crops inside the source slice. */
typedef struct unetk_lits_desc {
  int32_t N, H, W, C;
  int32_t n_slices, src_h, src_w; /* extent of the resident store; indices outside [0, n_slices) read as zeros */
  int32_t lab_scale; /* LB_SCALE = 64 */
  uint32_t seed;
  float noise_scale; /* 0 = no noise (eval_online) */
} unetk_lits_desc;
/* PNG row un-filtering for the resident slice store (the reference decodes with cv2 on tf.data threads,
 * DataLoader/Liver/input_pipeline.py:243-284; its PNGs come from SimpleITK / libpng with adaptive row filters,
 * DataLoader/Liver/extract.py:176-187).  filtered: n_images inflated IDAT streams of non-interlaced grayscale PNGs, image k at
 * filtered + k * image_stride_bytes, each h rows of (1 filter-type byte + w * bit_depth / 8 bytes).  out: image k at element
 * k * out_image_stride, h * w samples, uint8 (bit_depth 8) or native-endian uint16 (bit_depth 16).  All five filter types
 * (None, Sub, Up, Average, Paeth).  status[0] |= 1 if a row carries a filter type > 4 (the caller zeroes it and raises). */
int unetk_png_unfilter(const uint8_t* filtered, int64_t image_stride_bytes, int n_images, int h, int w, int bit_depth,
                       void* out, int64_t out_image_stride, int32_t* status, void* stream);
int unetk_lits_batch(const unetk_lits_desc* d, const uint16_t* slices, const uint8_t* seg_slices,
                     const int32_t* sample_tab, const float* clip, float* images, int32_t* labels,
                     void* stream);
/* Spatial guide of the guided LiTS pipeline (DataLoader/Liver/input_pipeline_g.py:382-412, utils/image_ops.py:396-434) for
 * a whole batch: per sample create_spatial_guide_2d(crop size, centres, max(stddevs, min_std)) -> resize_bilinear
 * (align_corners) to H x W -> g / 2 + 0.5, without rendering the crop-resolution guide: every output pixel evaluates
 * max_k exp(-((py - cy)^2 / (2 sy^2) + (px - cx)^2 / (2 sx^2))) at its 4 bilinear corners and lerps.  sample_tab is the
 * batch's unetk_lits_batch table (its crop box and flip columns are used, with the same clamp and flips, so guide and
 * image line up); obj_ptr int32 [N + 1] (CSR, entries clamped into [0, n_obj]); obj float [n_obj][4] = (cy, cx, sy, sx),
 * centres relative to the crop, in source pixels, 16-byte aligned (may be NULL when n_obj = 0); guide f32 [N, H, W, 1].
 * A sample without objects is exactly 0.5 (the reference's false_fn).  min_std > 0. */
typedef struct unetk_lits_guide_desc {
  int32_t N, H, W, C; /* C: image channels of sample_tab (rows of C + 7) */
  int32_t src_h, src_w;
  int32_t n_obj;
  float min_std; /* render-time stddev floor (1.0 in the reference) */
} unetk_lits_guide_desc;
int unetk_lits_spatial_guide(const unetk_lits_guide_desc* d, const int32_t* sample_tab, const int32_t* obj_ptr,
                             const float* obj, float* guide, void* stream);
/* Context rows of a batch of the guided LiTS pipeline (DataLoader/Liver/input_pipeline_g.py:527-550, :672-680):
 * out f32 [N, F] row s = table[sample_tab[s][C]] (the label-slice column of the unetk_lits_batch table), zeros where
 * take[s] == 0 (the guide coin failed) or the index is outside [0, n_rows) (padding, -1).  noise f64 [N, F] (NULL = none):
 * the resident row is first updated in place, row = f32(f64(row) + noise[s]), samples in order (the reference's noise
 * accumulates in its cached table).  table f32 [n_rows, F]. */
int unetk_lits_context(float* table, int64_t n_rows, int F, const int32_t* sample_tab, int N, int C, const int32_t* take,
                       const double* noise, float* out, void* stream);

/* ---------------------------------------------------------------- LiTS 3-D training patches  
 * UNet3D batches cropped from the resident slice store: the semantics of the reference's 3-D pipeline
 * (DataLoader/NF/input_pipeline_3d.py:544-604 gen_batch, :352-407 data_processing; DataLoader/misc.py:132-143 volume_crop;
 * utils/image_ops.py:241 random_flip, :339-354 augment_gamma) on LiTS volumes.
 *
 * sample_tab int32 [N][UNETK_LITS3D_TAB_COLS], one row per sample:
 *   0 base   store index of the case's first slice      8  flip_up_down
 *   1 depth  slices of the case                          9  flip_front_back
 *   2 cz     centre slice (within the case)              10 gamma (float bits; training only)
 *   3 cy     centre row                                  11 forced: 1 = (cy, cx) come from unetk_lits_pick_voxel
 *   4 cx     centre column                               12 k: rank of the forced-class pixel in slice cz
 *   5 ch     crop rows    = int32(H * zoom_y)            13, 14 sin, cos (float bits): read by the _rot / _warp entries only
 *   6 cw     crop columns = int32(W * zoom_x)            15 warp: != 0 = deformed; read by the _warp entries only
 *   7 flip_left_right
 *
 * unetk_lits_pick_voxel: for every row with forced != 0, (cy, cx) <- the k-th pixel, in row-major order, of slice
 *   base + cz with seg / lab_scale >= fg_label -- np.argwhere(lab[cz] >= fg_label)[k], exactly -- written into the table on
 *   the device.  Rows with forced == 0 are left alone.  A k outside [0, count) or a slice outside the store writes (0, 0)
 *   and sets status[0] |= 1 (the caller zeroes it); nothing is read out of bounds.  One block per sample.
 *
 * unetk_lits_patch3d: images f32 [N,D,H,W,1], labels int32 [N,D,H,W].  Per sample:
 *   crop box (volume_crop): ch, cw clamped into [1, src_h] x [1, src_w]; z1 = min(max(cz - D/2, 0), max(depth - D, 0)),
 *     y1 = min(max(cy - ch/2, 0), src_h - ch), x1 likewise; crop slices at or beyond `depth` (a case shallower than D)
 *     read as zeros with label 0;
 *   mask statistics over the crop at source resolution, v = stored / im_scale: mean m and standard deviation s over the
 *     voxels with v > 0 (fp64 partials per block, summed by index: bit-reproducible); an empty mask gives m = s = 0;
 *   image: every bilinear corner c is normalised on the fly, c > 0 ? (c - m) / (s + 1e-8) : 0, then resize_bilinear
 *     (align_corners) to H x W per slice -- normalise, then resize, as the reference;
 *   labels: resize_nearest_neighbor(align_corners), min(seg / lab_scale, lab_max);
 *   flips of image and label alike, by the write address;
 *   training != 0: augment_gamma(retain_stats=True) with the row's gamma: mn, sd, min, range of the patch,
 *     y = powf((x - min) / (range + 1e-7), gamma) * range + min, out = (y - mean(y) + mn) / (sd(y) + 1e-8) * sd.
 * D*H*W < 2^31 and D*src_h*src_w < 2^31 (else UNETK_E_UNSUPPORTED and a zero ws query); N <= 65535; ws 16-byte aligned, at
 * least unetk_lits_patch3d_ws_bytes (the partials and the per-sample statistics only). */
#define UNETK_LITS3D_TAB_COLS 16
typedef struct unetk_lits3d_desc {
  int32_t N, D, H, W;
  int32_t n_slices, src_h, src_w; /* extent of the resident store */
  int32_t im_scale, lab_scale;    /* IM_SCALE = LB_SCALE = 64 */
  int32_t lab_max;                /* labels are min(seg / lab_scale, lab_max): the number of foreground classes */
  int32_t training;               /* != 0: gamma augmentation */
} unetk_lits3d_desc;
int unetk_lits_pick_voxel(const uint8_t* seg_slices, int n_slices, int src_h, int src_w, int lab_scale, int fg_label,
                          int32_t* sample_tab, int N, int32_t* status, void* stream);
/* unetk_lits_pick_voxel_rows (additive to ABI 10): unetk_lits_pick_voxel for the rows whose column 11 EQUALS
 * forced_value (> 0) only, every other row is left alone -- so one table can hold rows centred on the label plane (value 1)
 * and rows centred on a second plane of the same extents and encoding (value 2: the `neg` plane of hard-negative training),
 * one call per plane.  A rank outside its slice's count writes (0, 0) and sets status[0] |= 1, and |= 2 as well when
 * forced_value > 1.  No other kernel reads column 11. */
int unetk_lits_pick_voxel_rows(const uint8_t* seg_slices, int n_slices, int src_h, int src_w, int lab_scale, int fg_label,
                               int32_t* sample_tab, int N, int32_t* status, int forced_value, void* stream);
size_t unetk_lits_patch3d_ws_bytes(const unetk_lits3d_desc* d);
int unetk_lits_patch3d(const unetk_lits3d_desc* d, const uint16_t* slices, const uint8_t* seg_slices,
                       const int32_t* sample_tab, float* images, int32_t* labels, void* ws, size_t ws_bytes, void* stream);

/* In-plane rotated patches (additive to ABI 10).  unetk_lits_patch3d with two more table columns:
 *   13 sin, 14 cos of the row's angle (float bits, formed by the host: the device never calls sincosf); 15 stays reserved.
 * A row whose columns 13 and 14 are BOTH bit-zero is not rotated: it takes the arithmetic of unetk_lits_patch3d and gives
 * its output bit for bit.  Any other content -- the explicit identity (0, 1) included -- is a rotated row:
 *   statistics: m, s over the UNROTATED crop box (pass 1 as it is); gamma as it is, on the rotated patch;
 *   coordinates: voxel (z, y, x) of the un-flipped patch samples crop slice z at, all float32, EVERY operation rounded on its
 *     own (no fused multiply-add: a numpy float32 restatement forms the same bits),
 *       hs = (ch - 1) / (H - 1), ws = (cw - 1) / (W - 1)  (0 for an axis of one voxel: align_corners)
 *       cy0 = 0.5 (ch - 1), cx0 = 0.5 (cw - 1);   u = y hs - cy0, v = x ws - cx0
 *       in_y = cy0 + (cos u - sin v),   in_x = cx0 + (sin u + cos v)
 *   image: i0 = floor(in_y), i1 = i0 + 1, f = in_y - i0, x likewise, the second tap NOT clamped; each of the four taps reads
 *     the SLICE at (y1 + i, x1 + j) where that lies inside [0, src_h) x [0, src_w) -- beyond the crop box there is real
 *     tissue -- and is 0 outside it; every tap is normalised on the fly as above, then the same lerps;
 *   labels: roundf of both coordinates; outside the slice 0, else min(seg / lab_scale, lab_max);
 *   a coordinate that is not finite or whose magnitude is >= 2^24 counts as outside: image 0, label 0.
 * Crop slices at or beyond the case's depth are zeros, the flips are the write address: as unetk_lits_patch3d.  Nothing is
 * read out of bounds for any table content.  Same arguments, checks, error codes and workspace query. */
int unetk_lits_patch3d_rot(const unetk_lits3d_desc* d, const uint16_t* slices, const uint8_t* seg_slices,
                           const int32_t* sample_tab, float* images, int32_t* labels, void* ws, size_t ws_bytes, void* stream);

/* Elastically deformed patches (additive to ABI 10).  unetk_lits_patch3d_rot with one more table column and
 * one more input:
 *   15 warp: 0 = the row is not deformed; anything else = it is, by its lattice;
 *   warp f32 [N][2][G + 3][G + 3]: per row the control displacements (0 = dy, 1 = dx, in pixels of the OUTPUT patch) of a
 *     uniform cubic B-spline with G x G cells across the patch, 1 <= G <= 16.  Rows with column 15 == 0 never read theirs.
 * A row with column 15 == 0 gives the output of unetk_lits_patch3d_rot bit for bit (and so, with columns 13 / 14 zero too, that of
 * unetk_lits_patch3d).  A deformed row, rotated or not -- all float32, EVERY operation rounded on its own:
 *   gy = H > 1 ? (float)G / (float)(H - 1) : 0;  t = y gy;  i = min((int)floor(t), G - 1);  f = t - i   (x: W, j, fx)
 *   g = 1 - f;  k6 = 1.f / 6.f
 *   w0 = ((g g) g) k6                               w1 = ((((3 f) - 6) f) f + 4) k6
 *   w2 = (((((-3 f) + 3) f + 3) f) + 1) k6          w3 = ((f f) f) k6
 *   dy = sum_a wy[a] (sum_b wx[b] warp[n][0][i + a][j + b]),  dx likewise from warp[n][1]; both sums left to right from term 0
 *   y' = y + dy,  x' = x + dx                       (the field is the same for every slice)
 *   not rotated: in_y = y' hs, in_x = x' ws;   rotated: u = y' hs - cy0, v = x' ws - cx0 and the sums of unetk_lits_patch3d_rot.
 * Everything else is the rotated row of unetk_lits_patch3d_rot: unclamped second tap, taps and label read from the SLICE and 0
 * outside it, labels roundf, m and s of the axis-aligned crop, gamma on the result, flips the write address, a coordinate that
 * is not finite or >= 2^24 in magnitude image 0 and label 0.  Nothing is read out of bounds for any table or lattice content.
 * warp NULL or misaligned, G outside [1, 16]: UNETK_E_BADARG.  Otherwise the arguments, checks, error codes and workspace query
 * of unetk_lits_patch3d_rot. */
int unetk_lits_patch3d_warp(const unetk_lits3d_desc* d, const uint16_t* slices, const uint8_t* seg_slices,
                            const int32_t* sample_tab, const float* warp, int G, float* images, int32_t* labels,
                            void* ws, size_t ws_bytes, void* stream);

/* Patches at a fixed slice spacing (additive to ABI 10).  unetk_lits_patch3d with one more input:
 *   zcrop int32 [N] (device memory, 4-byte aligned), zcrop_max (host int, >= 1): per row cd = min(max(zcrop[n], 1), zcrop_max)
 *   crop slices are resized to the D output slices -- a true 3-D crop-and-resize.
 * Per row:
 *   crop box: as unetk_lits_patch3d with cd in place of D, z1 = min(max(cz - cd/2, 0), max(depth - cd, 0)); cd is NOT clamped
 *     to the case: crop slices at or beyond `depth` read as zeros with label 0;
 *   mask statistics over the cd x ch x cw source crop (fp64 partials per block, summed by index);
 *   voxel (z, y, x) of the un-flipped patch: zs = (cd - 1) / (D - 1) (0 when D == 1), in_z = z zs (float32),
 *     i0 = floor(in_z), i1 = min(i0 + 1, cd - 1), fz = in_z - i0  -- the taps of y and x, align_corners;
 *   image: v0, v1 = the in-plane value of crop slices i0, i1, each computed exactly as unetk_lits_patch3d computes it (every
 *     corner normalised on the fly, then the two lerps; a slice outside the case gives 0), v = v0 + fz (v1 - v0);
 *     no anti-aliasing when cd > D, as in the plane;
 *   labels: crop slice min(roundf(in_z), cd - 1) at the in-plane nearest pixel;
 *   flips, patch moments and gamma as unetk_lits_patch3d, on the D x H x W result, same block partition.
 * A row with cd == D gives the output of unetk_lits_patch3d bit for bit (training != 0 included), whatever the other rows hold.
 * Nothing is read out of bounds for any content of zcrop.  zcrop NULL or misaligned, zcrop_max < 1: UNETK_E_BADARG;
 * zcrop_max * src_h * src_w >= 2^31: UNETK_E_UNSUPPORTED.  Otherwise the arguments, checks, error codes and workspace query of
 * unetk_lits_patch3d. */
int unetk_lits_patch3d_z(const unetk_lits3d_desc* d, const uint16_t* slices, const uint8_t* seg_slices,
                         const int32_t* sample_tab, const int32_t* zcrop, int zcrop_max, float* images, int32_t* labels,
                         void* ws, size_t ws_bytes, void* stream);

/* Whole-volume evaluation in windows.  probs f32 [N,D,H,W,C]: the class probabilities of the N windows that
 * unetk_lits_patch3d(training = 0) cut for sample_tab (same desc, same table, flips included).  acc f32 [depth,src_h,src_w,C],
 * cnt int32 [depth,src_h,src_w]: ONE case, zeroed by the caller before its first batch.  All rows must carry this case's
 * (base, depth).  For every voxel (z,y,x) of the case and every row n = 0..N-1 IN ORDER whose crop box holds it:
 *   acc[z,y,x,c] += resize_bilinear(align_corners) of probs[n,z - z1,:,:,c] from H x W to ch x cw, at (y - y1, x - x1),
 *   read through the row's flips;   cnt[z,y,x] += 1.
 * A gather: every (voxel, class) is written by one thread, rows are added in index order -- no atomics, two calls give
 * identical bits.  [z0,z1) x [y0,y1) x [x0,x1): the union box of the rows (the host knows it), the only voxels visited.
 * box = {z0, z1, y0, y1, x0, x1} (host memory), inside [0,depth) x [0,src_h) x [0,src_w) and not empty; 1 <= C <= 8; a row
 * whose (base, depth) differ from (case_base, case_depth) is rejected when the caller passes the table's host copy to the
 * wrapper (the entry point sees a device pointer), and contributes nothing on the device.  Window slices at or beyond
 * case_depth contribute nothing.  The size limits of unetk_lits_patch3d apply, and D*H*W*C < 2^31 (UNETK_E_UNSUPPORTED). */
int unetk_eval3d_accumulate(const unetk_lits3d_desc* d, const int32_t* sample_tab, const float* probs, int C,
                            int64_t case_base, int case_depth, const int32_t box[6], float* acc, int32_t* cnt, void* stream);

/* The same gather with centre-weighted windows (additive to ABI 10).  gz f32 [D], gy f32 [H], gx f32 [W]: the window's weight
 * per axis, indexed in the UN-FLIPPED window; wsum f32 [depth,src_h,src_w] takes the place of cnt.  Per hit
 *   w = gz[z - z1] * lerp(gy[y0], gy[y1], fy) * lerp(gx[x0], gx[x1], fx)      (lerp(a, b, f) = a + f (b - a))
 * with the taps and fractions of the probabilities' resize;  acc[z,y,x,c] += w * (the resized probability);  wsum[z,y,x] += w.
 * Same order, one writer per (voxel, class), no atomics, same checks and error codes; null or misaligned tables / wsum:
 * UNETK_E_BADARG.  All-ones tables give the acc of unetk_eval3d_accumulate bit for bit and wsum == cnt. */
int unetk_eval3d_accumulate_w(const unetk_lits3d_desc* d, const int32_t* sample_tab, const float* probs, int C,
                              int64_t case_base, int case_depth, const int32_t box[6], const float* gz, const float* gy,
                              const float* gx, float* acc, float* wsum, void* stream);

/* The way back of unetk_lits_patch3d_z (additive to ABI 10): the two gathers above for windows cut with the
 * same zcrop / zcrop_max pair.  A case voxel z lies in a row's window when 0 <= zw = z - z1 < cd (z1 with cd in place of D).
 * The inverse resize along z: in_z = zw (D - 1) / (cd - 1) (0 when cd == 1), i0 = floor(in_z), i1 = min(i0 + 1, D - 1),
 * fz = in_z - i0; the hit is p0 + fz (p1 - p0) of the in-plane bilerps p0, p1 of window slices i0 and i1, read through the row's
 * front/back flip.  _wz scales a hit by (gz[i0] + (gz[i1] - gz[i0]) fz) * wy * wx.  Rows in index order, one writer per
 * (voxel, class), no atomics; cnt and wsum as above.  When every row has cd == D the outputs equal those of
 * unetk_eval3d_accumulate / _w bit for bit.  zcrop NULL or misaligned, zcrop_max < 1: UNETK_E_BADARG; zcrop_max * src_h * src_w
 * >= 2^31: UNETK_E_UNSUPPORTED; nothing is read out of bounds for any content of zcrop. */
int unetk_eval3d_accumulate_z(const unetk_lits3d_desc* d, const int32_t* sample_tab, const int32_t* zcrop, int zcrop_max,
                              const float* probs, int C, int64_t case_base, int case_depth, const int32_t box[6], float* acc,
                              int32_t* cnt, void* stream);
int unetk_eval3d_accumulate_wz(const unetk_lits3d_desc* d, const int32_t* sample_tab, const int32_t* zcrop, int zcrop_max,
                               const float* probs, int C, int64_t case_base, int case_depth, const int32_t box[6],
                               const float* gz, const float* gy, const float* gx, float* acc, float* wsum, void* stream);

/* The end of a case: acc f32 [depth,src_h,src_w,C] and EXACTLY ONE of wsum (f32) / cnt (int32) [depth,src_h,src_w], the other
 * NULL -> pred uint8 [depth,src_h,src_w].  box = {z0, z1, y0, y1, x0, x1} (host memory, inside the volume, not empty): the part
 * of the case the windows tiled.  A voxel is covered when its weight is > 0;  pred = covered and inside box ? argmax over the
 * C sums (lowest index on ties, as unetk_head_predict) : 0 -- windows may reach beyond the box, what they leave there is not a
 * prediction.  *uncovered (int32, zeroed by the caller) += the voxels of box that are not covered, by integer atomics.
 * 1 <= C <= 8; depth * src_h * src_w < 2^31 (UNETK_E_UNSUPPORTED). */
int unetk_eval3d_finish(const float* acc, int C, int depth, int src_h, int src_w, const float* wsum, const int32_t* cnt,
                        const int32_t box[6], uint8_t* pred, int32_t* uncovered, void* stream);

/* The probability of ONE class of a sliding-window case as a saved volume (--pred_type prob; additive to ABI 10): acc, wsum / cnt
 * and box as unetk_eval3d_finish takes them, 0 <= c < C.  Per voxel p = acc[z,y,x,c] / weight in f32 (IEEE division, cnt
 * converted to f32), q = rint(255 * p) (ties to even) clamped to 0..255, and q = 0 where the weight is not > 0 or the voxel lies
 * outside box.  dst uint8 [depth * src_h * src_w] in NIfTI file order, (t0, t1, t2, flips) in unetk_nii_compose's convention;
 * every element is written exactly once, no workspace, two calls give identical bits.  One thread per file element: the stores
 * are consecutive bytes for every orientation; with t0 == 2 the reads walk consecutive voxels too (coalesced), for the other
 * orientations they are a plain per-element gather.  UNETK_E_BADARG: a NULL or misaligned pointer, both or neither weight,
 * C outside [1, 8], c outside [0, C), a box that is empty or leaves the volume, (t0, t1, t2) not a permutation;
 * UNETK_E_UNSUPPORTED: depth * src_h * src_w >= 2^31. */
int unetk_eval3d_prob(const float* acc, int C, int c, int depth, int src_h, int src_w, const float* wsum, const int32_t* cnt,
                      const int32_t box[6], int t0, int t1, int t2, int flips, uint8_t* dst, void* stream);

/* ---------------------------------------------------------------- LiTS click-guided 2-D batches  
 * Batches for the nets that take concat(images, sp_guide) (UNetInter, SmallUNet, InterUNet, LGNet), cropped from the resident
 * slice store with the semantics of the reference's interactive pipeline for the NF data (DataLoader/NF/
 * input_pipeline_g_simply.py:564-636 gen_batch, :435-527 data_processing, :346-412 inter_simulation as :530-561 gen_kernel
 * calls it; DataLoader/misc.py:108-129 img_crop; utils/image_ops.py:396-434 create_spatial_guide_2d).  Additive to ABI 10.
 *
 * sample_tab is the LiTS 3-D table (UNETK_LITS3D_TAB_COLS, same columns; flip_front_back is ignored), so
 * unetk_lits_pick_voxel runs on it unchanged.  The (y, x) crop box is unetk_lits_patch3d's: ch, cw clamped into
 * [1, src_h] x [1, src_w], y1 = min(max(cy - ch/2, 0), src_h - ch), x1 likewise.  Along z there is no clamp (img_crop):
 * channel c shows slice cz - C/2 + c of the case, zeros where that lies outside [0, depth) or the store (padding).  C odd.
 * The object is seg / lab_scale >= obj_label on slice cz.  status int32 [1] (zeroed by the caller) collects
 *   bit 1 (2): a row whose centre slice cz lies outside [0, depth) or the store -- its labels are 0, it has no object;
 *   bit 2 (4): a click_tab row out of range (n_fg outside [1, max_clicks), n_bg outside [0, max_clicks), a strategy other
 *              than 1 or 3) -- the value is clamped (strategy: 1).
 * Nothing is read out of bounds for any table content.
 *
 * unetk_lits_inter_batch: images f32 [N,H,W,C], labels int32 [N,H,W] in {0, 1}.  Per sample:
 *   mask statistics over the whole [C, ch, cw] crop at source resolution, v = stored / im_scale: mean m and standard deviation
 *     s of the voxels with v > 0 (fp64 partials per block, summed by index); an empty mask gives m = s = 0;
 *   image: every bilinear corner c is normalised on the fly, c > 0 ? (c - m) / (s + 1e-8) : 0, then resize_bilinear
 *     (align_corners) to H x W per channel;  labels: slice cz, resize_nearest_neighbor(align_corners), object ? 1 : 0;
 *   flips (left/right, up/down) of image and label alike, by the write address;
 *   training != 0: augment_gamma(retain_stats=True) with the row's gamma over the sample's whole [H,W,C] image, the
 *     arithmetic of unetk_lits_patch3d;  then, if noise_scale > 0:  v <- v + (2 u - 1) * noise_scale  with
 *     u = the library's counter generator (csrc/common.h, the dropout masks' one) of seed and the element's flat index in
 *     [N,H,W,C] taken modulo 2^32 (each operation rounded to float32 on its own), and
 *     every channel is multiplied by (max over (H, W) of that noised channel > 0 ? 1 : 0).
 *   H*W*C < 2^31, C*src_h*src_w < 2^31, C <= 7 (else UNETK_E_UNSUPPORTED and a zero ws query); N <= 65535; ws 16-byte aligned.
 *
 * unetk_lits_clicks: the click simulator.  pts int32 [N][2][UNETK_LITS_MAX_CLICKS][2] = (kind: 0 foreground / 1 background,
 *   click, (y, x) relative to the crop box; -1 padding), cnt int32 [N][2].  The object mask is the label crop at SOURCE
 *   resolution.  click_tab uint32 [N][UNETK_LITS_CLICK_TAB_COLS], the sample's draws:
 *     0 n_fg in [1, max_clicks)   1 n_bg in [0, max_clicks)   2 background strategy (1 or 3)   3 reserved (0)
 *     4..7 one 32-bit draw per foreground click                8..11 one per background click
 *   With d1 the city-block distance (binary_erosion's default cross, iterated):
 *     foreground candidates {p in obj : d1(p, background or outside the crop) > margin}      (border_value = 0)
 *     background candidates {p : margin < d1(p, obj) <= margin + band}                       (border_value = 1)
 *   A kind's mask is obj (foreground) / not obj (background).  A mask without a pixel gives no click (deviation: the
 *   reference would fail converting NaN for an all-object crop; it draws no foreground click without an object either).
 *   An empty candidate set ("small"): ONE click at (sum y / count, sum x / count) of the mask, integer floor division -- for
 *   the background without any object in the crop that is the crop's centre.  Otherwise up to n clicks: the first one, and
 *   every one under strategy 1, is the candidate of rank i = (r * count) >> 32 (64-bit integers, r the click's draw) in
 *   row-major order; under strategy 3 each later click is the candidate that maximises the minimum squared distance to the
 *   clicks so far, the first in row-major order on ties.  After a click the candidates with (y-cy)^2 + (x-cx)^2 <= step^2
 *   are removed; the kind stops early when none are left.  The foreground always uses strategy 1.
 *   margin, band >= 1, step >= 0, margin + band <= 254, 2 <= max_clicks <= UNETK_LITS_MAX_CLICKS + 1, src_h, src_w <= 1024
 *   (else UNETK_E_UNSUPPORTED and a zero ws query).  Integer arithmetic only, no atomics on results: two calls give
 *   identical bits.  ws: three byte fields of src_h * src_w per sample (column distances of both kinds, candidate classes).
 *
 * unetk_click_guide: guide f32 [N,H,W,G] from pts / cnt (plain device arrays: real clicks may be fed) and the sample table --
 *   same crop box and flips, so guide and image line up.  create_spatial_guide_2d at crop resolution, then resize_bilinear
 *   (align_corners), without the intermediate: every output pixel evaluates the guide at its 4 bilinear corners and lerps.
 *   gaussian == 0: min_k sqrt(dy^2 + dx^2) (not normalised);  gaussian != 0: max_k exp(-(dy^2 / (2 s^2) + dx^2 / (2 s^2))), s =
 *   stddev > 0.  A kind without clicks is exactly 0; cnt is clamped into [0, UNETK_LITS_MAX_CLICKS].  G == 2: (fg, bg);
 *   G == 1: fg - bg. */
#define UNETK_LITS_MAX_CLICKS 4
#define UNETK_LITS_CLICK_TAB_COLS 12
typedef struct unetk_lits_inter_desc {
  int32_t N, H, W, C;
  int32_t n_slices, src_h, src_w; /* extent of the resident store */
  int32_t im_scale, lab_scale;    /* IM_SCALE = LB_SCALE = 64 */
  int32_t obj_label;              /* object = seg / lab_scale >= obj_label */
  int32_t training;               /* != 0: gamma, noise, channel mask */
  uint32_t seed;
  float noise_scale;              /* 0 = no noise and no channel mask */
  int32_t margin, step, band, max_clicks; /* unetk_lits_clicks: the reference passes 3, 10, 40, 5 */
  int32_t G, gaussian;            /* unetk_click_guide */
  float stddev;
} unetk_lits_inter_desc;
size_t unetk_lits_inter_batch_ws_bytes(const unetk_lits_inter_desc* d);
int unetk_lits_inter_batch(const unetk_lits_inter_desc* d, const uint16_t* slices, const uint8_t* seg_slices,
                           const int32_t* sample_tab, float* images, int32_t* labels, int32_t* status, void* ws,
                           size_t ws_bytes, void* stream);
size_t unetk_lits_clicks_ws_bytes(const unetk_lits_inter_desc* d);
int unetk_lits_clicks(const unetk_lits_inter_desc* d, const uint8_t* seg_slices, const int32_t* sample_tab,
                      const uint32_t* click_tab, int32_t* pts, int32_t* cnt, int32_t* status, void* ws, size_t ws_bytes,
                      void* stream);
int unetk_click_guide(const unetk_lits_inter_desc* d, const int32_t* sample_tab, const int32_t* pts, const int32_t* cnt,
                      float* guide, void* stream);

/* ---------------------------------------------------------------- interactive evaluation: corrective clicks  
 * The click step of the reference's entry/main_eval.py (:149-183 inter_simulation_test) for N sessions at once, and the
 * guide from their click lists.  Additive to ABI 10.
 *
 * unetk_click_guide_list: unetk_click_guide from lists of K clicks per kind, pts int32 [N][2][K][2], cnt clamped into
 *   [0, K], 1 <= K <= UNETK_INTER_MAX_CLICKS.  Same kernel and arithmetic: with every count <= UNETK_LITS_MAX_CLICKS the
 *   output equals unetk_click_guide's bit for bit.
 *
 * unetk_inter_click: rows int32 [N][UNETK_INTER_ROW_COLS] = (slice index in the store, active != 0, previous click y, x; -1 =
 *   none).  pred uint8 [N][H][W] (non-zero = object) or NULL = all zeros.  vol uint8 [vol_depth][src_h][src_w] or NULL: the
 *   case's prediction volume, whose first slice is store slice vol_base.  pts int32 [N][2][K][2], cnt int32 [N][2]: the
 *   sessions' click lists (kind 0 foreground / 1 background), read and appended to.  Per active row:
 *     pred at source resolution, nearest: pixel (y, x) reads pred[y * H / src_h][x * W / src_w] (integer floor); it is written
 *       to slice (slice - vol_base) of vol;  ref = stored label >= obj_label * lab_scale;  err = pred xor ref;
 *     the 4-connected components of err; the largest one, the smallest root (= minimum linear index y * src_w + x) on ties;
 *     candidate = the component's mean per axis, rounded half to even (exact integers);
 *     click = the candidate where err is set there (err, not the component); otherwise (fallback) the component's pixel with
 *       the greatest city-block distance to the nearest non-error pixel, the slice's border counting as non-error, the
 *       distance capped at 255; ties: the smaller squared Euclidean distance to the candidate, then the smaller linear index;
 *     kind = ref set at the click ? 0 : 1;  repeat = the click equals the row's previous click;
 *     the click is appended to the kind's list unless the list holds K clicks already.
 *   An empty err gives no click (empty flag).  table int32 [N][UNETK_INTER_TAB_COLS]:
 *     0 n_pred  1 n_ref  2 n_inter (at source resolution)   3 components  4 area  5 root   6, 7 candidate (y, x)
 *     8, 9 click (y, x)  10 kind (-1 without a click)  11 fallback  12 repeat  13 empty  14 appended
 *     15 row state: 1 = ran, 0 = inactive, 2 = slice outside the store or the volume.  Rows in state 0 or 2 read and write
 *     nothing but their (otherwise zero) table row.
 *   src_h, src_w <= 1024, K <= UNETK_INTER_MAX_CLICKS, H * W < 2^21 (else UNETK_E_UNSUPPORTED and a zero ws query); N <= 65535;
 *   ws 16-byte aligned.  Integer arithmetic only; sums and maxima are integer atomics: two calls give identical bits. */
#define UNETK_INTER_MAX_CLICKS 64
#define UNETK_INTER_ROW_COLS 4
#define UNETK_INTER_TAB_COLS 16
typedef struct unetk_inter_click_desc {
  int32_t N, H, W;                /* sessions; extent of pred */
  int32_t n_slices, src_h, src_w; /* extent of the resident store */
  int32_t lab_scale, obj_label;   /* object = seg / lab_scale >= obj_label */
  int32_t K;                      /* clicks a list holds */
  int32_t vol_base, vol_depth;    /* vol[z] is store slice vol_base + z */
} unetk_inter_click_desc;
int unetk_click_guide_list(const unetk_lits_inter_desc* d, const int32_t* sample_tab, const int32_t* pts, const int32_t* cnt,
                           int K, float* guide, void* stream);
size_t unetk_inter_click_ws_bytes(const unetk_inter_click_desc* d);
int unetk_inter_click(const unetk_inter_click_desc* d, const uint8_t* seg_slices, const int32_t* rows, const uint8_t* pred,
                      uint8_t* vol, int32_t* pts, int32_t* cnt, int32_t* table, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- geodesic click guides  
 * The third guide kind of the click-guided nets (--geodesic_guide): the geodesic distance from the clicks through the image,
 * grown on the half-resolution centre channel (DataLoader/NF/input_pipeline_g_simply.py:471-496, entry/main_eval.py:205-220;
 * the reference calls GeodisTK's fast marching on the host).  Builder-defined, parity unpinned: the definition below is this
 * library's own.  Additive to ABI 10; unetk_lits_inter_desc is unchanged.  With hh = (H + 1) / 2, hw = (W + 1) / 2:
 *
 * unetk_lits_inter_center: the base field, base f32 [N][hh][hw].  base[n][i][j] is the value unetk_lits_inter_batch writes at
 *   pixel (2i, 2j) of channel C / 2 of sample n with training = 0 and the row's flip columns ignored -- img[::2, ::2, C // 2]
 *   of :484 -- bit for bit (same partial blocks, same expression).  Reads N, H, W, C, n_slices, src_h, src_w, im_scale of the
 *   desc; the checks, limits and status bit 1 (2) of unetk_lits_inter_batch.
 *
 * unetk_click_geodesic: guide f32 [N][H][W][G] from base (a plain device array: any field may be fed), the sample table (crop
 *   box and flips) and click lists pts int32 [N][2][K][2] = (kind, click, (y, x) relative to the crop box), cnt int32 [N][2]
 *   clamped into [0, K], 1 <= K <= UNETK_INTER_MAX_CLICKS.  Per sample and kind:
 *     seeds: gy = (int)(((float)y / (float)ch) * (float)H / 2.0f), gx likewise with cw and W (:483); each operation rounded to
 *       float32, truncation toward zero, the result clamped into the grid; duplicates are fine;
 *     D f32 [hh][hw]: the shortest-path distance on the 8-connected grid from the nearest seed under the step cost
 *       c(p, q) = sqrtf(s2 + (I[p] - I[q])^2), s2 = 1 for an axial step and 2 for a diagonal one, a path's length being the
 *       left-to-right float32 sum of its step costs from the seed; every operation is rounded to float32 on its own (no
 *       contraction), the square root correctly rounded.  Equivalently the fixed point with D = 0 at the seeds reached from
 *       +inf elsewhere under D[q] = min(D[q], min over the 8 neighbours p of fl(D[p] + c(p, q))): float addition is monotone and
 *       c >= 1, so every relaxation order ends at the same bits, those of a heap Dijkstra with the same operations;
 *     guide: resize_bilinear(align_corners) of D from hh x hw to H x W (:487), written through the row's flips; a kind without
 *       clicks is exactly 0;  G == 2: (fg, bg), G == 1: fg - bg; not normalised.
 *   dist f32 [N][2][hh][hw] or NULL receives the raw D (zeros for a kind without clicks).
 *   One workgroup solves one (sample, kind) from start to convergence inside one launch; no workgroup waits on another.
 *   unetk_click_geodesic_path: 0 = unsupported, 1 = I and D in LDS (at least 128 x 128 grids), 2 = I and D in the workspace
 *   (hh * hw <= 2^18); beyond that UNETK_E_UNSUPPORTED and a zero ws query.  The loop ends when a whole sweep lowers nothing and
 *   is bounded at hh * hw sweeps (Bellman-Ford: no order needs more); reaching the bound sets status bit 3 (8) and the launch
 *   ends normally.  The first N * 2 int32 words of ws hold the sweeps each solve ran (0 for a kind without clicks).
 *   Nothing is read or written out of bounds for any table or click content; two calls give identical bits.
 *   Reads N, H, W, src_h, src_w, G of the desc (the rest only has to be valid).  ws 16-byte aligned. */
size_t unetk_lits_inter_center_ws_bytes(const unetk_lits_inter_desc* d);
int unetk_lits_inter_center(const unetk_lits_inter_desc* d, const uint16_t* slices, const int32_t* sample_tab, float* base,
                            int32_t* status, void* ws, size_t ws_bytes, void* stream);
int unetk_click_geodesic_path(const unetk_lits_inter_desc* d);
size_t unetk_click_geodesic_ws_bytes(const unetk_lits_inter_desc* d);
int unetk_click_geodesic(const unetk_lits_inter_desc* d, const int32_t* sample_tab, const float* base, const int32_t* pts,
                         const int32_t* cnt, int K, float* guide, float* dist, int32_t* status, void* ws, size_t ws_bytes,
                         void* stream);

/* ---------------------------------------------------------------- LiTS 3-D click guides  
 * sp_guide for UNet3D: the clicks of the reference's 3-D pipeline (DataLoader/NF/input_pipeline_3d.py:258-324
 * inter_simulation as :474-504 gen_kernel calls it) simulated on the label patch of unetk_lits_patch3d, and rendered as
 * utils/image_ops.py:437-472 create_spatial_guide_3d renders them (:364-398 data_processing).  Additive to ABI 10.
 *
 * sample_tab is the LiTS 3-D table and the crop box is unetk_lits_patch3d's, z clamp included: the patch is [D, ch, cw], crop
 * slices at or beyond the case's depth (or outside the store) are label 0.  The object is seg / lab_scale >= obj_label.
 * click_tab is unetk_lits_clicks' table (UNETK_LITS_CLICK_TAB_COLS, same columns).  status int32 [1] (zeroed by the caller):
 *   bit 2 (4): a click_tab row out of range (n_fg outside [1, max_clicks), n_bg outside [0, max_clicks), a strategy other
 *              than 1 or 3) -- the value is clamped as unetk_lits_clicks clamps it (strategy: 1).
 * Nothing is read out of bounds for any table content.
 *
 * unetk_lits3d_clicks: pts int32 [N][2][UNETK_LITS_MAX_CLICKS][3] = (kind: 0 foreground / 1 background, click, (z, y, x) relative
 *   to the crop box; -1 padding), cnt int32 [N][2].  Three things differ from unetk_lits_clicks:
 *   1. The erosion's element is the 3 x 3 square of ONE slice (struct[1] = True), so with dinf the chessboard distance inside
 *      a slice -- nothing crosses slices:
 *        foreground candidates {p in obj : dinf(p, non-object of p's slice or outside the crop's (y, x) box) > margin}
 *        background candidates {p : margin < dinf(p, object of p's slice) <= margin + band}; a slice without an object has none
 *   2. Candidates are ordered (z, y, x) over the whole patch: a rank pick is i = (r * count) >> 32 in that order, and under
 *      strategy 3 a later click maximises the minimum squared 3-D distance dz^2 + dy^2 + dx^2 to the clicks so far, the
 *      first in (z, y, x) order on ties.  After a click only ITS OWN slice loses the candidates with dy^2 + dx^2 <= step^2.
 *      The kind stops when no candidate is left anywhere.
 *   3. "Small" (no candidate at all): ONE click at the mean of the kind's mask, rounded half to even per axis in integers
 *      (q = sum / n, r = sum % n: q if 2r < n, q + 1 if 2r > n, q + (q & 1) if 2r == n).
 *   The rest is unetk_lits_clicks': the draws, the foreground by rank, no foreground click without an object in the patch, a
 *   mask without a voxel gives no click (the deviation for an all-object patch).
 *   margin, band >= 1, step >= 0, margin + band <= 254, 2 <= max_clicks <= UNETK_LITS_MAX_CLICKS + 1, src_h, src_w <= 1024,
 *   D <= 256, D*src_h*src_w < 2^31, N <= 65535 (else UNETK_E_UNSUPPORTED and a zero ws query).  Integer arithmetic only, no
 *   atomics on results: two calls give identical bits.  ws (16-byte aligned): per sample three byte fields of D*src_h*src_w
 *   (rounded up to 16; column distances of both kinds, candidate classes), then int32 [N][D][src_h][8] row records
 *   (foreground candidates, background candidates, object pixels, sum of the object pixels' x, first and last x of a
 *   background candidate, two reserved).
 *
 * unetk_click_guide3d: guide f32 [N,D,H,W,G] from pts / cnt (plain device arrays: real clicks may be fed) -- same crop box and
 *   the three flips of unetk_lits_patch3d, so guide and image line up.  create_spatial_guide_3d at crop resolution [D, ch, cw],
 *   then resize_bilinear(align_corners) per slice, without the intermediate: every output voxel evaluates the guide at its 4
 *   in-plane bilinear corners and lerps.
 *   gaussian == 0: sqrt(min_k(dz^2 + dy^2 + dx^2)) / euclid_norm, euclid_norm > 0 formed by the caller (the reference divides by
 *     float32(im_height * sqrt(2) * 0.8));
 *   gaussian != 0: max_k exp(-(dz^2 / (2 sz^2) + dy^2 / (2 sy^2) + dx^2 / (2 sx^2))), summed z, y, x; stddev = {sz, sy, sx} > 0.
 *   A kind without clicks is exactly 0; cnt is clamped into [0, UNETK_LITS_MAX_CLICKS].  G == 2: (fg, bg); G == 1: fg - bg.
 *   D*H*W < 2^31 (else UNETK_E_UNSUPPORTED).  Reads D, H, W, src_h, src_w, G, gaussian, stddev, euclid_norm of the desc. */
typedef struct unetk_lits3d_clicks_desc {
  int32_t N, D, H, W;
  int32_t n_slices, src_h, src_w; /* extent of the resident store */
  int32_t lab_scale;              /* LB_SCALE = 64 */
  int32_t obj_label;              /* object = seg / lab_scale >= obj_label: the sampler's forced class */
  int32_t margin, step, band, max_clicks; /* the reference passes 3, 10, 40, 5 */
  int32_t G, gaussian;            /* unetk_click_guide3d */
  float stddev[3];                /* (z, y, x); --stddev, default 1 3 3 */
  float euclid_norm;
} unetk_lits3d_clicks_desc;
size_t unetk_lits3d_clicks_ws_bytes(const unetk_lits3d_clicks_desc* d);
int unetk_lits3d_clicks(const unetk_lits3d_clicks_desc* d, const uint8_t* seg_slices, const int32_t* sample_tab,
                        const uint32_t* click_tab, int32_t* pts, int32_t* cnt, int32_t* status, void* ws, size_t ws_bytes,
                        void* stream);
/* unetk_lits3d_clicks_neg (additive to ABI 10): unetk_lits3d_clicks with background clicks on false positives
 *   -- inter_simulation(strategy=4, neg_patch) as gen_kernel calls it under cfg.fp_sample.  neg_slices uint8
 *   [n_slices][src_h][src_w], a plane beside seg_slices in its encoding: a voxel is a false positive where neg / lab_scale >= 1;
 *   crop slices at or beyond the case's depth hold none.
 *   A row whose crop box holds no false positive is bit for bit a row of unetk_lits3d_clicks.  In a row whose crop holds one,
 *   the BACKGROUND kind's candidates are the crop's false-positive voxels -- no erosion, no band, whatever the label says there;
 *   n_bg clicks, EVERY one a rank pick i = (draw * count) >> 32 in (z, y, x) order over the candidates left; after a click only
 *   its own slice loses the candidates with dy^2 + dx^2 <= step^2; the kind stops when none is left.  No "small" click, and the
 *   row's strategy column is not used (an out-of-range value still sets bit 2).  The foreground kind is unchanged.  Limits,
 *   status bits, workspace (the query is unetk_lits3d_clicks_ws_bytes; the class bytes carry bit 3 and the row records' slot 6
 *   the row's false positives) and determinism as unetk_lits3d_clicks. */
int unetk_lits3d_clicks_neg(const unetk_lits3d_clicks_desc* d, const uint8_t* seg_slices, const uint8_t* neg_slices,
                            const int32_t* sample_tab, const uint32_t* click_tab, int32_t* pts, int32_t* cnt, int32_t* status,
                            void* ws, size_t ws_bytes, void* stream);
int unetk_click_guide3d(const unetk_lits3d_clicks_desc* d, const int32_t* sample_tab, const int32_t* pts, const int32_t* cnt,
                        float* guide, void* stream);

/* The guide of in-plane rotated patches (additive to ABI 10): unetk_click_guide3d that reads columns 13 / 14
 * of the table as unetk_lits_patch3d_rot does.  The clicks stay what unetk_lits3d_clicks simulates on the UNROTATED label crop
 * (relative to the crop box).  A row with both columns bit-zero gives the output of unetk_click_guide3d bit for bit.  A rotated
 * row evaluates the guide -- a function of position, defined beyond [0, ch) x [0, cw) too -- at the four unclamped corners
 * (i0 | i0 + 1, j0 | j0 + 1) of the in_y, in_x of unetk_lits_patch3d_rot (same float32 operations, no fused multiply-add) and
 * lerps them with the fractions in_y - i0, in_x - j0 as unetk_click_guide3d lerps its corners; where a coordinate is not finite
 * or its magnitude is >= 2^24 the guide is 0.  Every mode is served: Gaussian and Euclidean, G 1 and 2, the three flips; a
 * kind without clicks is exactly 0.  Same arguments, checks and error codes. */
int unetk_click_guide3d_rot(const unetk_lits3d_clicks_desc* d, const int32_t* sample_tab, const int32_t* pts, const int32_t* cnt,
                            float* guide, void* stream);

/* The guide of elastically deformed patches (additive to ABI 10): unetk_click_guide3d_rot that reads column 15
 * of the table and the lattices warp f32 [N][2][G + 3][G + 3] as unetk_lits_patch3d_warp does.  The clicks stay what
 * unetk_lits3d_clicks simulates on the UNDEFORMED label crop.  A row with column 15 == 0 gives the output of
 * unetk_click_guide3d_rot bit for bit.  A deformed row evaluates the guide at the four unclamped corners of the in_y, in_x of
 * unetk_lits_patch3d_warp (same float32 operations) and lerps them as unetk_click_guide3d_rot does; an invalid coordinate
 * gives 0.  warp NULL or misaligned, G (the lattice's; the descriptor's G is the guide's channels) outside [1, 16]:
 * UNETK_E_BADARG.  Otherwise the arguments, checks and error codes of unetk_click_guide3d_rot. */
int unetk_click_guide3d_warp(const unetk_lits3d_clicks_desc* d, const int32_t* sample_tab, const float* warp, int G,
                             const int32_t* pts, const int32_t* cnt, float* guide, void* stream);

/* ---------------------------------------------------------------- 3-D interactive evaluation: corrective clicks  
 * The click step of the reference's entry/main_eval_3d.py (:152-185 inter_simulation_test) for ONE case, and the guide of the
 * case's windows from its click lists.  Additive to ABI 10.
 *
 * unetk_click_guide3d_list: unetk_click_guide3d for the N rows of a LiTS 3-D table from ONE pair of click lists shared by all
 *   rows: pts int32 [2][K][3] = (kind, click, (z, y, x)) in CASE coordinates -- z from the case's first slice, (y, x) in the
 *   slice -- and cnt int32 [2], clamped into [0, K]; 1 <= K <= UNETK_INTER_MAX_CLICKS (else UNETK_E_BADARG).  Per row the crop
 *   box's origin (z1, y1, x1) is subtracted from the clicks in integers; a click outside the box takes part with its true
 *   (negative or large) offset.  Then the same kernel and arithmetic: unetk_click_guide3d fed the clicks relative to the row's
 *   box, with counts <= UNETK_LITS_MAX_CLICKS, gives the same output bit for bit.
 *
 * unetk_inter_click3d: the case is the `depth` store slices from `case_base`; a voxel's linear index is (z * src_h + y) * src_w
 *   + x with z from the case's first slice.  pred uint8 [depth][src_h][src_w] (non-zero = object) or NULL = all zeros.
 *   (prev_z, prev_y, prev_x): the previous click, -1 = none.  pts int32 [2][K][3], cnt int32 [2]: the case's click lists in case
 *   coordinates (kind 0 foreground / 1 background), read and appended to.
 *     ref = stored label >= obj_label * lab_scale;  err = pred xor ref;
 *     the 6-connected components of err; the largest one, the smallest root (= minimum linear index) on ties;
 *     candidate = the component's mean per axis, rounded half to even (exact integers, the q / r rule of unetk_lits3d_clicks);
 *     click = the candidate where err is set there (err, not the component); otherwise (fallback) the component's voxel with
 *       the greatest 3-D city-block distance to the nearest non-error voxel, the case's border counting as non-error, the
 *       distance capped at dist_cap; ties: the smaller squared Euclidean distance to the candidate, then the smaller index;
 *     kind = ref set at the click ? 0 : 1;  repeat = the click equals the previous click;
 *     the click is appended to the kind's list unless the list holds K clicks already.
 *   An empty err gives no click (empty flag).  table int32 [UNETK_INTER3D_TAB_COLS]:
 *     0 n_pred  1 n_ref  2 n_inter   3 components  4 area  5 root   6, 7, 8 candidate (z, y, x)   9, 10, 11 click (z, y, x)
 *     12 kind   13 fallback  14 repeat  15 empty  16 appended   17 row state: 1 = ran, 2 = the case leaves the store (nothing
 *     but the row is written)   18, 19 zero.  Columns 5 .. 12 are -1 without a click.
 *   src_h, src_w <= 1024, depth <= 4096 (the fallback's key holds the squared distance to the candidate in 25 bits),
 *   depth * src_h * src_w < 2^31, K <= UNETK_INTER_MAX_CLICKS (else UNETK_E_UNSUPPORTED and a zero ws query); 1 <= dist_cap <= 255;
 *   ws 16-byte aligned.  Integer arithmetic only; sums and maxima are integer atomics: two calls give identical bits.  Nothing
 *   is written beyond pts, cnt, the table row and ws. */
#define UNETK_INTER3D_TAB_COLS 20
typedef struct unetk_inter_click3d_desc {
  int32_t case_base, depth;       /* the case: store slices [case_base, case_base + depth) */
  int32_t n_slices, src_h, src_w; /* extent of the resident store */
  int32_t lab_scale, obj_label;   /* object = seg / lab_scale >= obj_label */
  int32_t K;                      /* clicks a list holds */
  int32_t dist_cap;               /* cap of the fallback's distance, 1 .. 255 */
} unetk_inter_click3d_desc;
int unetk_click_guide3d_list(const unetk_lits3d_clicks_desc* d, const int32_t* sample_tab, const int32_t* pts, const int32_t* cnt,
                             int K, float* guide, void* stream);
size_t unetk_inter_click3d_ws_bytes(const unetk_inter_click3d_desc* d);
int unetk_inter_click3d(const unetk_inter_click3d_desc* d, const uint8_t* seg_slices, const uint8_t* pred, int prev_z, int prev_y,
                        int prev_x, int32_t* pts, int32_t* cnt, int32_t* table, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- slice prior of click-guided UNet3D  
 * The second image channel of the reference's --use_cascade without --use_2d (DataLoader/NF/input_pipeline_3d.py:505-533
 * gen_kernel, :411-471 data_processing_2c; entry/main_eval_3d.py:348-369): what the object looks like on the slice z0 of the
 * first foreground click.  Additive to ABI 10.  The descriptor is unetk_lits3d_clicks_desc, of which N, D, H, W, the store's
 * extent, lab_scale and obj_label are read, sample_tab the LiTS 3-D table, the object seg / lab_scale >= obj_label.
 *
 * unetk_slice_prior_field: per table row n an int32 field over a box of ONE store slice, and z0 int32 [N].
 *   z0: K == 0: pts int32 [N][2][UNETK_LITS_MAX_CLICKS][3], cnt int32 [N][2] (what unetk_lits3d_clicks gives):
 *         z0[n] = cnt[n][0] > 0 ? pts[n][0][0][0] : -1;
 *       1 <= K <= UNETK_INTER_MAX_CLICKS: ONE pair of lists pts int32 [2][K][3], cnt int32 [2] (unetk_inter_click3d's): every
 *         row takes z0 = cnt[0] > 0 ? pts[0][0][0] : -1.  The value is written to z0[n] as read.
 *   box: whole == 0: the row's crop box of unetk_lits_patch3d, bh x bw = ch x cw at (y1, x1), and z0 counts from the box's
 *         first slice z1 -- the slice is crop slice z0 where 0 <= z0 < D;
 *       whole != 0: the whole slice, bh x bw = src_h x src_w at (0, 0), and z0 counts from the case's first slice.
 *     Without a click, with z0 outside that range, on a crop slice at or beyond the case's depth or outside the store, the mask
 *     is all background.  Otherwise mask(i, j) = object at (y1 + i, x1 + j) of that slice.
 *   field int32 [N][src_h * src_w]: row n's box is stored densely at the start of its plane, pixel (i, j) at i * bw + j; the
 *     rest of the plane is not written.
 *   mode UNETK_SLICE_PRIOR_BINARY: field = mask (0 / 1).
 *   mode UNETK_SLICE_PRIOR_BOUNDARY: a foreground pixel is BOUNDARY when at least one of its 4-neighbours INSIDE the box is
 *     background; the border of the box does not count as background.  (skimage find_boundaries(mode="inner"): dilation !=
 *     erosion under the cross footprint, ANDed with the foreground -- a neighbour beyond the border never changes a pixel's
 *     own value under either border rule skimage has used, minimum / maximum padding or reflection.)
 *     field = D2(i, j) = min over boundary pixels (i', j') of (i - i')^2 + (j - j')^2, exact integers -- the squared Euclidean
 *     distance transform, in two separable passes: g(i, j) = distance along row i to its nearest boundary pixel (capped at
 *     32768 where the row has none), then D2(i, j) = min over i' of (i - i')^2 + g(i', j)^2.  With src_h, src_w <= 4096
 *     (else UNETK_E_UNSUPPORTED and a zero ws query) nothing exceeds 2^30 + 4111^2 < 2^31.
 *     Because every seed of the reference's 3-D transform lies in slice z0, its distance is exactly sqrt(dz^2 + D2).
 *   SENTINEL: a box without a boundary pixel -- no click, no object on the slice, or an object that fills the box -- gets
 *     field = -1 everywhere, which renders as exactly 0.  Deviation 1 from the scipy / skimage corner cases: the reference feeds
 *     zeros only for "no click"; with an empty boundary it calls distance_transform_edt on an array without a seed, whose
 *     answer is an artefact of scipy's implementation -- here the rule is: no boundary, no prior.  Deviation 2: a crop slice
 *     at or beyond the case's depth (a case shallower than D is padded with label-0 slices, as unetk_lits_patch3d pads it) is
 *     background, where the reference's crop would have indexed from a negative start.
 *   ws (16-byte aligned, boundary mode only; NULL is fine for binary): int32 [N][src_h * src_w], the g^2 of the row pass.
 *   Integer arithmetic, no atomics: two calls give identical bits.  Nothing is read out of bounds for any table or click
 *   content.  N <= 65535.
 *
 * unetk_slice_prior_render: images2 f32 [N,D,H,W,2] (8-byte aligned) from images f32 [N,D,H,W,1] = what unetk_lits_patch3d
 *   wrote for the same table, and field / z0 as above.
 *   channel 0 = images, copied bit for bit (so no concat pass follows);
 *   channel 1 = the prior: create-then-resize as unetk_click_guide3d -- the value at crop resolution is v(z, i, j), evaluated
 *     at the four in-plane corners (i0 | i1, j0 | j1) of resize_bilinear(align_corners) from ch x cw to H x W and lerped,
 *       in_y = y * ((ch - 1) / (H - 1)), i0 = min(floor(in_y), ch - 1), i1 = min(floor(in_y) + 1, ch - 1), ly = in_y - floor(in_y)
 *       top = tl + (tr - tl) lx,  bot = bl + (br - bl) lx,  out = top + (bot - top) ly
 *     in float32 with EVERY operation rounded on its own (no fused multiply-add: a float32 restatement forms the same taps);
 *     boundary: v = D2[i][j] < 0 ? 0 : expf(-sqrtf((float)(dz dz + D2[i][j])) / 25.f)     binary: v = dz == 0 ? mask[i][j] : 0
 *     the three flips of the table are the write address, as for the image.  No z-score, no gamma, no noise touches channel 1:
 *     data_processing_2c splits the prior off before the z-score and re-attaches it after the gamma.
 *   shared == 0: field [N][src_h * src_w] per row over its crop box (whole == 0 above), z0 [N], dz = z - z0[n].
 *   shared != 0: ONE field over the whole slice (whole != 0 above, the plane of row 0) and ONE z0 [1], both in case coordinates,
 *     for all N rows of a window table: each row reads pixel (y1 + i, x1 + j) and dz = z1 + z - z0[0] -- its box origin
 *     subtracted in integers; dz may be negative or exceed D.  Fed the crop of the same field, the per-row form gives the
 *     same bits.
 *   D*H*W < 2^31 (else UNETK_E_UNSUPPORTED). */
#define UNETK_SLICE_PRIOR_BOUNDARY 0
#define UNETK_SLICE_PRIOR_BINARY 1
size_t unetk_slice_prior_ws_bytes(const unetk_lits3d_clicks_desc* d);
int unetk_slice_prior_field(const unetk_lits3d_clicks_desc* d, const uint8_t* seg_slices, const int32_t* sample_tab,
                            const int32_t* pts, const int32_t* cnt, int K, int whole, int mode, int32_t* field, int32_t* z0,
                            void* ws, size_t ws_bytes, void* stream);
int unetk_slice_prior_render(const unetk_lits3d_clicks_desc* d, const int32_t* sample_tab, const float* images,
                             const int32_t* field, const int32_t* z0, int shared, int mode, float* images2, void* stream);

/* ---------------------------------------------------------------- optimiser  core/solver.py:204-243
 * tf.train.AdamOptimizer on a flat parameter buffer.  g' = g*gscale + l2*p  (slim.l2_regularizer
 * gradient, base.py:128-135);  m += (1-b1)(g'-m);  v += (1-b2)(g'^2-v);
 * p -= lr_t * m / (sqrt(v) + eps)  with lr_t = lr*sqrt(1-b2^t)/(1-b1^t) computed by the caller.
 * decoupled_wd > 0 = tf.contrib.opt.AdamWOptimizer (solver.py:212-216): p <- p*(1 - wd) first. */
int unetk_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr_t,
                    float beta1, float beta2, float eps, float gscale, float l2, float decoupled_wd,
                    void* stream);
/* tf.train.MomentumOptimizer: acc = mom*acc + g'; p -= lr*acc (nesterov: lr*(g' + mom*acc)). */
int unetk_momentum_step(float* p, const float* g, float* acc, int64_t n, float lr, float mom,
                        int nesterov, float gscale, float l2, void* stream);
/* out[0] = sum(p^2) (fp64 accumulate) -- for the reported regularisation loss. ws >= 8 KiB. */
int unetk_sumsq(const float* p, int64_t n, float* out, void* ws, size_t ws_bytes, void* stream);

/* tf.train.NanTensorHook(loss) (core/estimator.py:676: every step, raises NanLossDuringTrainingError) without a host sync
 * per step: if value[0] is NaN and flag[0] == 0, set flag[0] = 1 and flag[1] = step (sticky; the caller zeroes flag[0..1]
 * once and reads it whenever it synchronises anyway: log steps, and before every checkpoint it writes). */
int unetk_nan_watch(const float* value, int32_t* flag, int32_t step, void* stream);

/* ---------------------------------------------------------------- kernel trace (measurement only; bench.py)
 * SURVEY.md 8d asks for the dominant kernel's launch duration "measured live inside bench.py with HIP events ... on the
 * stream the kernel is launched on".  The reference has no counterpart (its profiling is tf.train.ProfilerHook,
 * core/estimator.py:688-690).  While enabled, EVERY kernel this library launches carries a start / stop event pair bound to
 * the dispatch (hipExtLaunchKernelGGL), i.e. the GPU's own begin -> end interval of that kernel -- what rocprofv3
 * --kernel-trace reports -- independent of host gaps around the launch.  Process-wide diagnostic state, off by default; the
 * only exception to the "no global mutable state" rule above.  No call here synchronises.
 *   unetk_prof_reset(n)     forget all records; pre-create events for n launches (outside any timed region)
 *   unetk_prof_enable(on)   start / stop recording (records accumulate across enable periods until the next reset)
 *   unetk_prof_mark()       number of launches recorded so far: a caller brackets one ABI call with two marks
 *   unetk_prof_read(...)    durations in ms of records [first, first + count); the stream must have been synchronised
 *                           (else hipErrorNotReady is returned)
 *   unetk_prof_name(i,...)  demangled kernel name of record i, as rocprofv3 prints it */
int unetk_prof_reset(int reserve_launches);
int unetk_prof_enable(int on);
int unetk_prof_mark(void);
int unetk_prof_read(int first, int count, float* ms_out);
int unetk_prof_name(int i, char* buf, int cap);

#ifdef __cplusplus
}
#endif
#endif /* UNETK_H_ */
