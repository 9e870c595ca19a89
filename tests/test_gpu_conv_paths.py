"""The 3x3 convolution family (forward with statistic partials, input gradient, filter gradient) on every dispatch path,
with inputs for which fp32 arithmetic is exact in any summation order.

`x` holds small integers in [-4, 4], `w` eighths in [-2/8, 2/8], `dy` integers in [-2, 2]: every product and every partial sum
is a multiple of 1/8 (1 for dw) far below 2^24 of those units, so whatever tile, split, stream-K cut or MFMA order a kernel
uses, its result equals the float64 convolution bit for bit; bf16 holds these inputs exactly as well.  Each row asserts the two
bounds that keep it in that regime (max(|x| conv |w|) * 8 < 2^24 and 8 * N * H * W < 2^24) from its own inputs.  A second,
sparse input set (x, w in {-1, 0, 1}, density chosen so that max |y| <= 15) makes the statistic partials exact too.

Each row of CASES names the kernels it exists to reach (forward, input gradient, filter gradient, and the same for UNETK_BF16 /
UNETK_BF16S where unetk_conv_bf16_ok admits the row), written out by hand from the plan parts of csrc/conv_igemm.hip (tiled_bn,
small_grid, big_grid, unetk_conv_plan), csrc/conv_igemm_lin.hip (lin_ok, lin_bm, sk_plan), csrc/conv_wgrad.hip (unetk_wgrad_plan,
launch_plan), csrc/conv_igemm_bf16.hip (pick_bf16), csrc/conv_igemm_bf16s.hip (unetk_conv_plan_bf16s_v3) and
csrc/conv_wgrad_bf16s.hip (unetk_wgrad_plan_bf16s).  The library's launch trace must show exactly those kernels, so a row that lands elsewhere
after a dispatch change fails instead of quietly testing something else.  `None` = the entry point refuses the shape (the row
then skips that op; test_refusals covers the refusals themselves).

Gaussian inputs keep the bounds of test_gpu_ops.py unchanged: 2e-6 forward, 3e-6 dx / dw, 1e-5 dw from 100 k pixels on.
Three rows cannot hold the forward bound for fp32 arithmetic alone: the plain linear-pixel kernel with K = 9 Cin = 6768 .. 9072
products per output in one fp32 chain (the exact tier shows these very launches bit-equal to float64).  They carry the rule of
test_gpu_head.py's header, 4 x the error of the same convolution evaluated in torch float32 on the CPU against float64 on that
row's Gaussian inputs (GAUSS_Y_TOL; measured CPU errors 3.45e-6, 3.00e-6, 3.35e-6; the kernel's own: 3.60e-6, 3.39e-6, 3.22e-6).

The same Gaussian tier runs under UNETK_BF16 (float64 reference on the bf16-rounded operands; 3e-6 y / dx, 5e-6 dw, 1e-5 dw
from 100 k pixels on, statistics 3e-4 / 3e-5: test_gpu_bf16.py) and UNETK_BF16S (stored values within one bf16 ulp of the exact
result and all but 2e-3 of them its exact rounding, dw 1e-5 / 2e-5, statistics 3e-5: test_gpu_bf16s.py).  No row carries an override there: the
UNETK_BF16 kernels hold 3e-6 on the Cin = 512 .. 1024 rows as well (measured 0.9e-6 .. 1.2e-6).

Limits: channel-slice views (xpad / ypad) run in the fp32 and UNETK_BF16 tiers; under UNETK_BF16S the rows run dense, except
test_bf16s_tall_tile_with_a_4_channel_y_pad, because most pads of the table are not multiples of the 8 channels that mode's
16-byte units need.  conv3x3_wgrad_bf16s_kernel<false> is reachable only through the UNETK_WGRAD_DEEP measurement switch and
has no row.  The bench brackets of ops.py take their tag from this same trace (the first launch inside the bracket):
test_bench_bracket_tag_is_the_first_traced_kernel.

Small rows take the float64 reference from oracle/tf_ops.conv_nd_same on the CPU, rows marked big=True from the same function
on the device (it is F.conv2d in float64 there).
"""
import collections
import ctypes

import pytest
import torch

from oracle import tf_ops
import guardbuf

pytestmark = pytest.mark.gpu

E_BADARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3
FP32, BF16, BF16S = 0, 1, 2
PREC_NAME = {FP32: "fp32", BF16: "bf16", BF16S: "bf16s"}

Case = collections.namedtuple("Case", "id n h w cin cout rows fwd dgrad wgrad dil xpad ypad big sk bf16 bf16s")


def _c(id, n, h, w, cin, cout, rows, fwd, dgrad, wgrad, dil=1, xpad=0, ypad=0, big=False, sk=False, bf16=None, bf16s=None):
    return Case(id, n, h, w, cin, cout, rows, fwd, dgrad, wgrad, dil, xpad, ypad, big, sk, bf16, bf16s)


# id, N, H, W, Cin, Cout, statistic rows of the fp32 forward,
#   fp32 forward kernels, fp32 input-gradient kernels, fp32 filter-gradient kernels,
#   bf16 / bf16s = (forward kernels, statistic rows, input-gradient kernels, filter-gradient kernels)
# xpad / ypad: x (dy) is a channel slice of a buffer xpad (ypad) channels wider and y (dx) is written into such a slice
# sk: the row also runs three ways through the C ABI (test_stream_k_workspace_three_ways)
CASES = [
    # ---- tiled kernel, 128-wide: 4-row (small_grid), 8-row, 16-row (big_grid) tiles on both sides of the cut-offs
    _c("t4_ragged", 2, 22, 40, 32, 128, 36,
       ["conv3x3_igemm_kernel<2,2,1,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<4>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 18, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<4>"]), xpad=8, ypad=4),
    _c("t4_b383", 383, 8, 16, 32, 128, 766,
       ["conv3x3_igemm_kernel<2,2,1,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<16>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 383, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<16>"])),
    _c("t8_b384", 384, 8, 16, 32, 128, 384,
       ["conv3x3_igemm_kernel<2,2,2,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<16>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 384, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<16>"])),
    _c("t8_w15", 384, 8, 15, 32, 128, 384,
       ["conv3x3_igemm_kernel<2,2,2,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<16>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 384, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<16>"])),
    _c("t8_ragged", 8, 70, 100, 32, 128, 504,
       ["conv3x3_igemm_kernel<2,2,2,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<16>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 504, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<16>"]), big=True),
    _c("t8_big511", 7, 16, 1160, 32, 128, 1022,
       ["conv3x3_igemm_kernel<2,2,2,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<16>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 1022, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<16>"]), big=True),
    _c("t16_big512", 8, 16, 1020, 32, 128, 512,
       ["conv3x3_igemm_kernel<2,2,4,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<16>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 1024, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<16>"]), big=True),
    _c("t16_w15", 512, 16, 15, 32, 128, 512,
       ["conv3x3_igemm_kernel<2,2,4,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<16>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 1024, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<16>"]), big=True),
    _c("t8_c256", 5, 104, 128, 256, 256, 520,
       ["conv3x3_igemm_kernel<2,2,2,2,1,1,0>"], ["conv3x3_igemm_kernel<2,2,2,2,1,1,0>"],
       ["conv3x3_wgrad_kernel<64,64,false,8,16,false,1,1>", "slab_reduce_kernel<4>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,2,4,2,false,false,false>"], 160, ["conv3x3_igemm_bf16_kernel<4,2,4,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>", "slab_reduce_kernel<4>"]),
       bf16s=(["conv3x3_bf16s_kernel<8,false,0>"], 160, ["conv3x3_bf16s_kernel<8,false,0>"], ["conv3x3_wgrad_bf16s_kernel<true>", "slab_reduce_kernel<4>"]), big=True),
    # ---- tiled kernel, 64-wide (8- and 16-row) and 32-wide
    _c("n64t8_ragged", 2, 20, 40, 32, 64, 18,
       ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<4>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,2,2,false,false,false>"], 12, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<4>"]), xpad=4, ypad=12),
    _c("n64t8_w15", 2, 8, 15, 64, 64, 2,
       ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"],
       ["conv3x3_wgrad_kernel<64,64,false,8,16,false,1,1>", "slab_reduce_kernel<1>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], 2, ["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>", "slab_reduce_kernel<1>"]),
       bf16s=(["conv3x3_igemm_bf16_kernel<4,1,1,2,true,false,false>"], 2, ["conv3x3_igemm_bf16_kernel<4,1,1,2,true,false,false>"], ["conv3x3_wgrad_bf16s_kernel<true>", "slab_reduce_kernel<1>"])),
    _c("n64t8_big511", 7, 16, 1160, 32, 64, 1022,
       ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<16>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,2,2,false,false,false>"], 511, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<16>"]), big=True),
    _c("n64t16_big512", 8, 16, 1020, 32, 64, 512,
       ["conv3x3_igemm_kernel<4,1,2,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<16>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,2,2,false,false,false>"], 512, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<16>"]), big=True),
    _c("n64t16_w15", 512, 16, 15, 32, 64, 512,
       ["conv3x3_igemm_kernel<4,1,2,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<16>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,2,2,false,false,false>"], 512, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<16>"]), big=True),
    _c("n32_ragged", 2, 20, 40, 32, 32, 12,
       ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,32,false,8,16,false,1,1>", "slab_reduce_kernel<4>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], 12, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,32,true,8,16,false,1,1>", "slab_reduce_kernel<4>"]), xpad=4, ypad=4),
    _c("n32_w7", 1, 5, 7, 32, 32, 1,
       ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,32,false,8,16,false,1,1>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], 1, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,32,true,8,16,false,1,1>"])),
    _c("n32_co96", 1, 17, 33, 64, 96, 6,
       ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"], ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"],
       ["conv3x3_wgrad_kernel<64,32,false,8,16,false,1,1>", "slab_reduce_kernel<4>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], 6, ["conv3x3_igemm_bf16_kernel<4,1,2,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,32,true,8,16,false,1,1>", "slab_reduce_kernel<4>"])),
    # ---- atrous (dilation 2)
    _c("atrous128", 2, 20, 24, 64, 128, 12,
       ["conv3x3_igemm_kernel<2,2,2,2,1,2,0>"], ["conv3x3_igemm_kernel<4,1,1,2,1,2,0>"],
       ["conv3x3_wgrad_kernel<64,64,false,6,16,false,1,2>", "slab_reduce_kernel<4>"], dil=2, xpad=4, ypad=8),
    _c("atrous64", 2, 20, 24, 64, 64, 12,
       ["conv3x3_igemm_kernel<4,1,1,2,1,2,0>"], ["conv3x3_igemm_kernel<4,1,1,2,1,2,0>"],
       ["conv3x3_wgrad_kernel<64,64,false,6,16,false,1,2>", "slab_reduce_kernel<4>"], dil=2),
    _c("atrous64_1x1", 3, 1, 1, 64, 64, 3,
       ["conv3x3_igemm_kernel<4,1,1,2,1,2,0>"], ["conv3x3_igemm_kernel<4,1,1,2,1,2,0>"],
       ["conv3x3_wgrad_kernel<64,64,false,6,16,false,1,2>", "slab_reduce_kernel<1>"], dil=2),
    _c("atrous128_2x3", 3, 2, 3, 64, 128, 3,
       ["conv3x3_igemm_kernel<2,2,2,2,1,2,0>"], ["conv3x3_igemm_kernel<4,1,1,2,1,2,0>"],
       ["conv3x3_wgrad_kernel<64,64,false,6,16,false,1,2>", "slab_reduce_kernel<1>"], dil=2),
    # ---- linear-pixel kernel, plain
    _c("lin_w1", 1, 200, 1, 32, 64, 2,
       ["conv3x3_igemm_lin_kernel<4,1,1,2,false,false,false,false,false,false>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<4>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,2,2,false,false,false>"], 13, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<4>"])),
    _c("lin_w2", 3, 30, 2, 32, 64, 3,
       ["conv3x3_igemm_lin_kernel<4,1,1,2,false,false,false,false,false,false>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<4>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,2,2,false,false,false>"], 6, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<4>"])),
    _c("lin_w3", 2, 21, 3, 32, 128, 2,
       ["conv3x3_igemm_lin_kernel<2,2,1,2,false,false,false,false,false,false>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<1>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 6, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<1>"])),
    _c("lin_w31", 2, 9, 31, 32, 64, 6,
       ["conv3x3_igemm_lin_kernel<4,1,1,2,false,false,false,false,false,false>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<4>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], 8, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<4>"]), xpad=4, ypad=4),
    _c("lin_p45", 7, 9, 5, 64, 64, 7,
       ["conv3x3_igemm_lin_kernel<4,1,1,2,false,false,false,false,false,false>"], ["conv3x3_igemm_lin_kernel<4,1,1,2,false,false,false,false,false,false>"],
       ["conv3x3_wgrad_kernel<64,64,false,8,16,false,1,1>", "slab_reduce_kernel<4>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], 14, ["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>", "slab_reduce_kernel<4>"]),
       bf16s=(["conv3x3_igemm_bf16_kernel<4,1,1,2,true,false,false>"], 14, ["conv3x3_igemm_bf16_kernel<4,1,1,2,true,false,false>"], ["conv3x3_wgrad_bf16s_kernel<true>", "slab_reduce_kernel<4>"])),
    _c("lin_p45_bm64", 3, 9, 5, 32, 128, 3,
       ["conv3x3_igemm_lin_kernel<2,2,1,2,false,false,false,false,false,false>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<1>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 6, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<1>"])),
    _c("t4_p144", 5, 12, 12, 64, 128, 15,
       ["conv3x3_igemm_kernel<2,2,1,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"],
       ["conv3x3_wgrad_kernel<64,64,false,10,12,true,1,1>", "slab_reduce_kernel<1>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 10, ["conv3x3_igemm_bf16_kernel<4,1,2,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>", "slab_reduce_kernel<4>"]),
       bf16s=(["conv3x3_igemm_bf16_kernel<2,2,2,2,true,false,false>"], 10, ["conv3x3_igemm_bf16_kernel<4,1,2,2,true,false,false>"], ["conv3x3_wgrad_bf16s_kernel<true>", "slab_reduce_kernel<4>"])),
    _c("n64_p36", 9, 6, 6, 64, 64, 9,
       ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"],
       ["conv3x3_wgrad_kernel<64,64,false,20,6,true,1,1>", "slab_reduce_kernel<1>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], 9, ["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>", "slab_reduce_kernel<4>"]),
       bf16s=(["conv3x3_igemm_bf16_kernel<4,1,1,2,true,false,false>"], 9, ["conv3x3_igemm_bf16_kernel<4,1,1,2,true,false,false>"], ["conv3x3_wgrad_bf16s_kernel<true>", "slab_reduce_kernel<4>"])),
    _c("lin128_24", 2, 24, 24, 64, 128, 18,
       ["conv3x3_igemm_lin_kernel<2,2,1,2,false,false,false,false,false,false>"], ["conv3x3_igemm_lin_kernel<4,1,1,2,false,false,false,false,false,false>"],
       ["conv3x3_wgrad_kernel<64,64,false,10,12,true,1,1>", "slab_reduce_kernel<4>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 12, ["conv3x3_igemm_bf16_kernel<4,1,2,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>", "slab_reduce_kernel<4>"]),
       bf16s=(["conv3x3_igemm_bf16_kernel<2,2,2,2,true,false,false>"], 12, ["conv3x3_igemm_bf16_kernel<4,1,2,2,true,false,false>"], ["conv3x3_wgrad_bf16s_kernel<true>", "slab_reduce_kernel<4>"])),
    _c("lin_starved", 1, 8, 16, 64, 128, 2,
       ["conv3x3_igemm_lin_kernel<2,2,1,2,false,false,false,false,false,false>"], ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"],
       ["conv3x3_wgrad_kernel<64,64,false,8,16,false,1,1>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 1, ["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>"]),
       bf16s=(["conv3x3_igemm_bf16_kernel<2,2,2,2,true,false,false>"], 1, ["conv3x3_igemm_bf16_kernel<4,1,1,2,true,false,false>"], ["conv3x3_wgrad_bf16s_kernel<true>"])),
    _c("lin_starved256", 128, 8, 16, 32, 128, 128,
       ["conv3x3_igemm_lin_kernel<2,2,2,2,false,false,true,false,false,false>", "lin_sk_fixup_kernel<128,128>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<16>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 128, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<16>"])),
    _c("t4_starved258", 129, 8, 16, 32, 128, 258,
       ["conv3x3_igemm_kernel<2,2,1,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<16>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 129, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<16>"])),
    _c("t4_gpix120", 1, 8, 15, 64, 128, 2,
       ["conv3x3_igemm_kernel<2,2,1,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"],
       ["conv3x3_wgrad_kernel<64,64,false,8,16,false,1,1>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 1, ["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>"]),
       bf16s=(["conv3x3_igemm_bf16_kernel<2,2,2,2,true,false,false>"], 1, ["conv3x3_igemm_bf16_kernel<4,1,1,2,true,false,false>"], ["conv3x3_wgrad_bf16s_kernel<true>"])),
    # ---- linear-pixel kernel, stream-K (three ways through the C ABI)
    _c("sk128", 8, 16, 16, 256, 128, 16,
       ["conv3x3_igemm_lin_kernel<2,2,2,2,false,false,true,false,false,false>", "lin_sk_fixup_kernel<128,128>"], ["conv3x3_igemm_lin_kernel<2,2,2,2,false,false,true,false,false,false>", "lin_sk_fixup_kernel<128,128>"],
       ["conv3x3_wgrad_kernel<64,64,false,8,16,false,1,1>", "slab_reduce_kernel<4>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 16, ["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>", "slab_reduce_kernel<4>"]),
       bf16s=(["conv3x3_igemm_bf16_kernel<2,2,2,2,true,false,false>"], 16, ["conv3x3_igemm_bf16_kernel<2,2,2,2,true,false,false>"], ["conv3x3_wgrad_bf16s_kernel<true>", "slab_reduce_kernel<4>"]), sk=True, ypad=4),
    _c("sk64", 2, 8, 8, 1024, 128, 2,
       ["conv3x3_igemm_lin_kernel<2,2,1,2,false,false,true,false,false,false>", "lin_sk_fixup_kernel<64,128>"], ["conv3x3_igemm_lin_kernel<2,2,1,2,false,false,true,false,false,false>", "lin_sk_fixup_kernel<64,128>"],
       ["conv3x3_wgrad_kernel<64,64,false,8,16,false,1,1>", "slab_reduce_kernel<1>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 2, ["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>", "slab_reduce_kernel<1>"]),
       bf16s=(["conv3x3_igemm_bf16_kernel<2,2,2,2,true,false,false>"], 2, ["conv3x3_igemm_bf16_kernel<2,2,2,2,true,false,false>"], ["conv3x3_wgrad_bf16s_kernel<true>", "slab_reduce_kernel<1>"]), sk=True),
    _c("sk64_tot126", 2, 8, 8, 1008, 128, 2,
       ["conv3x3_igemm_lin_kernel<2,2,1,2,false,false,false,false,false,false>"], None,
       None, sk=True),
    _c("sk128x64", 9, 9, 9, 512, 64, 9,
       ["conv3x3_igemm_lin_kernel<4,1,1,2,false,false,true,false,false,false>", "lin_sk_fixup_kernel<128,64>"], ["conv3x3_igemm_lin_kernel<2,2,1,2,false,false,true,false,false,false>", "lin_sk_fixup_kernel<64,128>"],
       ["conv3x3_wgrad_kernel<64,64,false,8,16,false,1,1>", "slab_reduce_kernel<4>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], 18, ["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>", "slab_reduce_kernel<4>"]),
       bf16s=(["conv3x3_igemm_bf16_kernel<4,1,1,2,true,false,false>"], 18, ["conv3x3_igemm_bf16_kernel<2,2,2,2,true,false,false>"], ["conv3x3_wgrad_bf16s_kernel<true>", "slab_reduce_kernel<4>"]), sk=True),
    _c("sk_t256", 256, 9, 9, 32, 64, 256,
       ["conv3x3_igemm_lin_kernel<4,1,1,2,false,false,true,false,false,false>", "lin_sk_fixup_kernel<128,64>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<16>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], 512, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<16>"]), sk=True),
    _c("sk_t257", 257, 9, 9, 32, 64, 257,
       ["conv3x3_igemm_lin_kernel<4,1,1,2,false,false,false,false,false,false>"], ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"],
       ["conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "slab_reduce_kernel<16>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], 514, ["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], ["conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "slab_reduce_kernel<16>"]), sk=True),
    _c("sk_nc48", 400, 9, 9, 768, 64, 400,
       ["conv3x3_igemm_lin_kernel<4,1,1,2,false,false,true,false,false,false>", "lin_sk_fixup_kernel<128,64>"], ["conv3x3_igemm_lin_kernel<2,2,2,2,false,false,false,false,false,false>"],
       ["conv3x3_wgrad_kernel<64,64,false,8,16,false,1,1>", "slab_reduce_kernel<4>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], 800, ["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>", "slab_reduce_kernel<4>"]),
       bf16s=(["conv3x3_igemm_bf16_kernel<4,1,1,2,true,false,false>"], 800, ["conv3x3_igemm_bf16_kernel<2,2,2,2,true,false,false>"], ["conv3x3_wgrad_bf16s_kernel<true>", "slab_reduce_kernel<4>"]), sk=True, big=True),
    _c("sk_nc47", 400, 9, 9, 752, 64, 400,
       ["conv3x3_igemm_lin_kernel<4,1,1,2,false,false,false,false,false,false>"], None,
       None, sk=True, big=True),
    # ---- filter-gradient plans
    _c("wg_1tile", 1, 8, 16, 64, 64, 1,
       ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"],
       ["conv3x3_wgrad_kernel<64,64,false,8,16,false,1,1>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], 1, ["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>"]),
       bf16s=(["conv3x3_igemm_bf16_kernel<4,1,1,2,true,false,false>"], 1, ["conv3x3_igemm_bf16_kernel<4,1,1,2,true,false,false>"], ["conv3x3_wgrad_bf16s_kernel<true>"])),
    _c("wg_64_32", 3, 9, 17, 64, 32, 6,
       ["conv3x3_igemm_kernel<4,1,2,1,1,1,0>"], ["conv3x3_igemm_lin_kernel<4,1,1,2,false,false,false,false,false,false>"],
       ["conv3x3_wgrad_kernel<64,32,false,8,16,false,1,1>", "slab_reduce_kernel<4>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>"], 6, ["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,32,true,8,16,false,1,1>", "slab_reduce_kernel<4>"])),
    _c("wg_stk6", 70, 6, 6, 128, 128, 140,
       ["conv3x3_igemm_kernel<2,2,1,2,1,1,0>"], ["conv3x3_igemm_kernel<2,2,1,2,1,1,0>"],
       ["conv3x3_wgrad_kernel<64,64,false,20,6,true,1,1>", "slab_reduce_kernel<4>"],
       bf16=(["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], 70, ["conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>", "slab_reduce_kernel<4>"]),
       bf16s=(["conv3x3_igemm_bf16_kernel<2,2,2,2,true,false,false>"], 70, ["conv3x3_igemm_bf16_kernel<2,2,2,2,true,false,false>"], ["conv3x3_wgrad_bf16s_kernel<true>", "slab_reduce_kernel<4>"])),
    _c("wg_stk12", 7, 24, 12, 64, 64, 21,
       ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"],
       ["conv3x3_wgrad_kernel<64,64,false,10,12,true,1,1>", "slab_reduce_kernel<4>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,2,2,false,false,false>"], 14, ["conv3x3_igemm_bf16_kernel<4,1,2,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>", "slab_reduce_kernel<4>"]),
       bf16s=(["conv3x3_igemm_bf16_kernel<4,1,2,2,true,false,false>"], 14, ["conv3x3_igemm_bf16_kernel<4,1,2,2,true,false,false>"], ["conv3x3_wgrad_bf16s_kernel<true>", "slab_reduce_kernel<4>"]), xpad=4, ypad=4),
    _c("wg_s5", 5, 8, 16, 64, 64, 5,
       ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"],
       ["conv3x3_wgrad_kernel<64,64,false,8,16,false,1,1>", "slab_reduce_kernel<1>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], 5, ["conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>", "slab_reduce_kernel<1>"]),
       bf16s=(["conv3x3_igemm_bf16_kernel<4,1,1,2,true,false,false>"], 5, ["conv3x3_igemm_bf16_kernel<4,1,1,2,true,false,false>"], ["conv3x3_wgrad_bf16s_kernel<true>", "slab_reduce_kernel<1>"])),
    # ---- first layers: matrix-pipe kernel (Cout = 64, Cin 1..5), direct kernels, their filter gradients
    _c("c3_ci1", 2, 13, 21, 1, 64, 8,
       ["conv3x3_c3_mfma_kernel<1,float,false>"], None,
       ["conv3x3_wgrad_c3_kernel<64>", "slab_reduce_kernel<4>"]),
    _c("c3_ci2", 2, 13, 21, 2, 64, 8,
       ["conv3x3_c3_mfma_kernel<2,float,false>"], None,
       ["conv3x3_wgrad_c3_kernel<64>", "slab_reduce_kernel<4>"]),
    _c("c3_ci3", 2, 13, 21, 3, 64, 8,
       ["conv3x3_c3_mfma_kernel<3,float,false>"], None,
       ["conv3x3_wgrad_c3_kernel<64>", "slab_reduce_kernel<4>"], xpad=2, ypad=4),
    _c("c3_ci4", 2, 13, 21, 4, 64, 8,
       ["conv3x3_c3_mfma_kernel<4,float,false>"], None,
       ["conv3x3_wgrad_smallc_kernel<4>", "slab_reduce_kernel<4>"]),
    _c("c3_ci5", 2, 13, 21, 5, 64, 8,
       ["conv3x3_c3_mfma_kernel<5,float,false>"], None,
       ["conv3x3_wgrad_smallc_kernel<5>", "slab_reduce_kernel<4>"]),
    _c("direct_ci1_co4", 1, 9, 17, 1, 4, 4,
       ["conv3x3_direct_kernel<1,float>"], None,
       ["conv3x3_wgrad_smallc_kernel<1>", "slab_reduce_kernel<1>"]),
    _c("direct_ci1_co32", 1, 9, 17, 1, 32, 4,
       ["conv3x3_direct_kernel<1,float>"], None,
       ["conv3x3_wgrad_c3_kernel<32>", "slab_reduce_kernel<1>"]),
    _c("direct_ci1_co128", 1, 9, 17, 1, 128, 4,
       ["conv3x3_direct_kernel<1,float>"], None,
       ["conv3x3_wgrad_smallc_kernel<1>", "slab_reduce_kernel<1>"]),
    _c("direct_ci2_co4", 1, 9, 17, 2, 4, 4,
       ["conv3x3_direct_kernel<2,float>"], None,
       ["conv3x3_wgrad_smallc_kernel<2>", "slab_reduce_kernel<1>"]),
    _c("direct_ci2_co32", 1, 9, 17, 2, 32, 4,
       ["conv3x3_direct_kernel<2,float>"], None,
       ["conv3x3_wgrad_c3_kernel<32>", "slab_reduce_kernel<1>"], xpad=1, ypad=4),
    _c("direct_ci2_co128", 1, 9, 17, 2, 128, 4,
       ["conv3x3_direct_kernel<2,float>"], None,
       ["conv3x3_wgrad_smallc_kernel<2>", "slab_reduce_kernel<1>"]),
    _c("direct_ci3_co4", 1, 9, 17, 3, 4, 4,
       ["conv3x3_direct_kernel<3,float>"], None,
       ["conv3x3_wgrad_smallc_kernel<3>", "slab_reduce_kernel<1>"]),
    _c("direct_ci3_co32", 1, 9, 17, 3, 32, 4,
       ["conv3x3_direct_kernel<3,float>"], None,
       ["conv3x3_wgrad_c3_kernel<32>", "slab_reduce_kernel<1>"]),
    _c("direct_ci3_co128", 1, 9, 17, 3, 128, 4,
       ["conv3x3_direct_kernel<3,float>"], None,
       ["conv3x3_wgrad_smallc_kernel<3>", "slab_reduce_kernel<1>"]),
    _c("direct_ci4_co4", 1, 9, 17, 4, 4, 4,
       ["conv3x3_direct_kernel<4,float>"], None,
       ["conv3x3_wgrad_smallc_kernel<4>", "slab_reduce_kernel<1>"]),
    _c("direct_ci4_co32", 1, 9, 17, 4, 32, 4,
       ["conv3x3_direct_kernel<4,float>"], None,
       ["conv3x3_wgrad_smallc_kernel<4>", "slab_reduce_kernel<1>"]),
    _c("direct_ci4_co128", 1, 9, 17, 4, 128, 4,
       ["conv3x3_direct_kernel<4,float>"], None,
       ["conv3x3_wgrad_smallc_kernel<4>", "slab_reduce_kernel<1>"]),
    _c("direct_ci5_co4", 1, 9, 17, 5, 4, 4,
       ["conv3x3_direct_kernel<5,float>"], None,
       ["conv3x3_wgrad_smallc_kernel<5>", "slab_reduce_kernel<1>"]),
    _c("direct_ci5_co32", 1, 9, 17, 5, 32, 4,
       ["conv3x3_direct_kernel<5,float>"], None,
       ["conv3x3_wgrad_smallc_kernel<5>", "slab_reduce_kernel<1>"]),
    _c("direct_ci5_co128", 1, 9, 17, 5, 128, 4,
       ["conv3x3_direct_kernel<5,float>"], None,
       ["conv3x3_wgrad_smallc_kernel<5>", "slab_reduce_kernel<1>"]),
    _c("direct0_ci6_co20", 2, 7, 19, 6, 20, 4,
       ["conv3x3_direct_kernel<0,float>"], None,
       None, xpad=3),
    _c("direct0_ci8_co36", 2, 7, 19, 8, 36, 4,
       ["conv3x3_direct_kernel<0,float>"], None,
       None),
    _c("direct0_ci12_co100", 2, 7, 19, 12, 100, 4,
       ["conv3x3_direct_kernel<0,float>"], None,
       None),
    _c("direct0_ci20_co4", 2, 7, 19, 20, 4, 4,
       ["conv3x3_direct_kernel<0,float>"], None,
       None),
    _c("direct0_ci9_co64", 2, 10, 18, 9, 64, 8,
       ["conv3x3_direct_kernel<0,float>"], None,
       ["conv3x3_wgrad_smallc_kernel<9>", "slab_reduce_kernel<4>"]),
    # ---- the persistent bf16-storage kernel at Cout = 64 (its 128-wide form is reached by t8_c256)
    _c("bf16s_v3_64", 8, 64, 208, 64, 64, 832,
       ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"], ["conv3x3_igemm_kernel<4,1,1,2,1,1,0>"],
       ["conv3x3_wgrad_kernel<64,64,false,8,16,false,1,1>", "slab_reduce_kernel<16>"],
       bf16=(["conv3x3_igemm_bf16_kernel<4,1,2,2,false,false,false>"], 416, ["conv3x3_igemm_bf16_kernel<4,1,2,2,false,false,false>"], ["conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>", "slab_reduce_kernel<16>"]),
       bf16s=(["conv3x3_bf16s_kernel<4,false,0>"], 208, ["conv3x3_bf16s_kernel<4,false,0>"], ["conv3x3_wgrad_bf16s_kernel<true>", "slab_reduce_kernel<16>"]), big=True),
]
BY_ID = {c.id: c for c in CASES}

# every kernel the table has to reach (the names as the launch trace prints them, blanks removed)
REQUIRED = [
    # tiled forward / input gradient
    "conv3x3_igemm_kernel<2,2,1,2,1,1,0>", "conv3x3_igemm_kernel<2,2,2,2,1,1,0>", "conv3x3_igemm_kernel<2,2,4,2,1,1,0>",
    "conv3x3_igemm_kernel<4,1,1,2,1,1,0>", "conv3x3_igemm_kernel<4,1,2,2,1,1,0>", "conv3x3_igemm_kernel<4,1,2,1,1,1,0>",
    # atrous
    "conv3x3_igemm_kernel<2,2,2,2,1,2,0>", "conv3x3_igemm_kernel<4,1,1,2,1,2,0>",
    # linear-pixel kernel, plain and stream-K
    "conv3x3_igemm_lin_kernel<2,2,1,2,false,false,false,false,false,false>",
    "conv3x3_igemm_lin_kernel<2,2,2,2,false,false,false,false,false,false>",
    "conv3x3_igemm_lin_kernel<4,1,1,2,false,false,false,false,false,false>",
    "conv3x3_igemm_lin_kernel<2,2,1,2,false,false,true,false,false,false>",
    "conv3x3_igemm_lin_kernel<2,2,2,2,false,false,true,false,false,false>",
    "conv3x3_igemm_lin_kernel<4,1,1,2,false,false,true,false,false,false>",
    "lin_sk_fixup_kernel<64,128>", "lin_sk_fixup_kernel<128,128>", "lin_sk_fixup_kernel<128,64>",
    # first layers
    "conv3x3_c3_mfma_kernel<1,float,false>", "conv3x3_c3_mfma_kernel<2,float,false>", "conv3x3_c3_mfma_kernel<3,float,false>",
    "conv3x3_c3_mfma_kernel<4,float,false>", "conv3x3_c3_mfma_kernel<5,float,false>",
    "conv3x3_direct_kernel<0,float>", "conv3x3_direct_kernel<1,float>", "conv3x3_direct_kernel<2,float>",
    "conv3x3_direct_kernel<3,float>", "conv3x3_direct_kernel<4,float>", "conv3x3_direct_kernel<5,float>",
    # filter gradient
    "conv3x3_wgrad_kernel<64,64,false,8,16,false,1,1>", "conv3x3_wgrad_kernel<64,32,false,8,16,false,1,1>",
    "conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>", "conv3x3_wgrad_kernel<32,32,false,8,16,false,1,1>",
    "conv3x3_wgrad_kernel<64,64,false,10,12,true,1,1>", "conv3x3_wgrad_kernel<64,64,false,20,6,true,1,1>",
    "conv3x3_wgrad_kernel<64,64,false,6,16,false,1,2>", "conv3x3_wgrad_c3_kernel<64>", "conv3x3_wgrad_c3_kernel<32>",
    "conv3x3_wgrad_smallc_kernel<1>", "conv3x3_wgrad_smallc_kernel<2>", "conv3x3_wgrad_smallc_kernel<3>",
    "conv3x3_wgrad_smallc_kernel<4>", "conv3x3_wgrad_smallc_kernel<5>", "conv3x3_wgrad_smallc_kernel<9>",
    "slab_reduce_kernel<16>", "slab_reduce_kernel<4>", "slab_reduce_kernel<1>",
    # reduced precision
    "conv3x3_igemm_bf16_kernel<4,2,4,2,false,false,false>", "conv3x3_igemm_bf16_kernel<2,2,2,2,false,false,false>",
    "conv3x3_igemm_bf16_kernel<4,1,2,2,false,false,false>", "conv3x3_igemm_bf16_kernel<4,1,1,2,false,false,false>",
    "conv3x3_igemm_bf16_kernel<4,1,2,1,false,false,false>",
    "conv3x3_igemm_bf16_kernel<2,2,2,2,true,false,false>", "conv3x3_igemm_bf16_kernel<4,1,2,2,true,false,false>",
    "conv3x3_igemm_bf16_kernel<4,1,1,2,true,false,false>", "conv3x3_igemm_bf16_kernel<4,2,4,2,true,false,false>",
    "conv3x3_bf16s_kernel<8,false,0>", "conv3x3_bf16s_kernel<4,false,0>",
    "conv3x3_wgrad_kernel<64,64,true,8,16,false,1,1>", "conv3x3_wgrad_kernel<64,32,true,8,16,false,1,1>",
    "conv3x3_wgrad_kernel<32,64,true,8,16,false,1,1>", "conv3x3_wgrad_kernel<32,32,true,8,16,false,1,1>",
    "conv3x3_wgrad_bf16s_kernel<true>", "conv3x3_wgrad_c3_bf16s_kernel(",
    "conv3x3_c3_mfma_kernel<1,unsignedshort,false>", "conv3x3_c3_mfma_kernel<2,unsignedshort,false>",
    "conv3x3_c3_mfma_kernel<3,unsignedshort,false>",
]
# filter-gradient plans (unetk_wgrad_plan): row -> (splits S of the fp32 launch, splits of the UNETK_BF16 launch where the row has
# that tier, what the row is there for).  unetk_conv3x3_wgrad_ws_bytes reads the plan of the launch the descriptor names -- its
# precision and dilation included -- and asks for exactly 256 + S x 9 Cin Cout x 4 bytes, so every S is asserted against the
# library, and against the reducer the row's trace names (S >= 64: <16>, 8 .. 63: <4>, 2 .. 7: <1>, 1: none).  UNETK_BF16 has
# no stacked-plane tiles: on those rows it splits the plain 8 x 16 tiles.
WG_PLANS = {
    "t4_b383": (128, 128, "one-round branch (256 / 2 panels); 383 tiles = 127 splits of 3 + one of 2: ragged last split"),
    "t8_big511": (128, 128, "one-round branch; 1022 tiles = 127 splits of 8 + one of 6: ragged last split"),
    "n32_ragged": (18, 18, "18 tiles, one each"),
    "wg_1tile": (1, 1, "one tile: S == 1, dw written in place, no reducer in the trace"),
    "t4_gpix120": (1, 1, "one tile"),
    "wg_s5": (5, 5, "five tiles, five splits: slab_reduce_kernel<1>"),
    "t8_c256": (31, 31, "total_tiles / S >= 16: the two-round plan (512 / 16 panels = 32 -> 31 splits of 17 tiles, the last has 10)"),
    "lin128_24": (10, 12, "stacked 10 x 12: N (H + 1) = 50 rows -> 5 tile rows x 2 columns; bf16: 2 x 3 x 2 plain tiles"),
    "wg_stk12": (18, 21, "stacked 10 x 12: N (H + 1) = 175 rows -> 18 tile rows, the last half empty, planes cross tiles; bf16: 7 x 3 x 1"),
    "wg_stk6": (25, 35, "stacked 20 x 6: N (H + 1) = 490 rows -> 25 tile rows, the last half empty; bf16: 70 plain tiles, "
                        "one round of 256 / 4 panels = 64 -> 35 splits of 2"),
    "atrous128": (16, None, "6 x 16 tiles: 2 x 4 x 2 = 16, one each (512 / 2 panels wanted, floor)"),
    "atrous64": (16, None, "6 x 16 tiles: 16, one each"),
    "atrous64_1x1": (3, None, "one tile per image"),
    "atrous128_2x3": (3, None, "one tile per image"),
}

# forward bound of the Gaussian tier where fp32 arithmetic alone exceeds 2e-6 (see the module docstring): 4 x the CPU float32 error
GAUSS_Y_TOL = {
    "sk64_tot126": 4 * 3.446e-6,      # Cin = 1008, plain 64-pixel linear kernel
    "sk_nc48": 4 * 3.003e-6,          # Cin = 768: the 256 whole tiles of the stream-K launch run their K loop in one piece
    "sk_nc47": 4 * 3.352e-6,          # Cin = 752, plain 128-pixel linear kernel
}

TRACED = {}            # (row id, input set) -> set of traced kernel names (blanks removed)
EXACT_STATS = {}       # forward kernel name -> ids of the rows whose two statistic sums were compared exactly


@pytest.fixture(scope="module")
def ops():
    from boxsegliver_amd import ops as _ops
    from boxsegliver_amd import _abi
    _abi.lib()
    return _ops


def lib():
    from boxsegliver_amd import _abi
    return _abi.lib()


def _p(t):
    return None if t is None else ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _trace(ops, fn):
    ops.profile_begin(0)
    ops.profile_on([])
    try:
        out = fn()
    finally:
        ops.profile_on(None)
    torch.cuda.synchronize()
    return out, [_norm(n) for n in ops.profile_read()[1]]


def _norm(name):
    return name.replace(" ", "").replace("(anonymousnamespace)::", "")


def _assert_trace(names, expect, what):
    """The traced launches are exactly the expected kernels, in order (a pack kernel is not part of the op)."""
    got = [n for n in names if "pack_" not in n]
    assert len(got) == len(expect) and all(e in g for e, g in zip(expect, got)), "{}: traced {} expected {}".format(what, got, expect)


def _seed(case, kind):
    return 7000 + sum(ord(ch) for ch in case.id) + {"eighths": 0, "sparse": 1, "gauss": 2}[kind]


def make_inputs(case, kind):
    """CPU float32 x [N,H,W,Cin], w [3,3,Cin,Cout], dy [N,H,W,Cout] and the unit (lsb) of y."""
    g = torch.Generator().manual_seed(_seed(case, kind))
    xs, ws, ys = (case.n, case.h, case.w, case.cin), (3, 3, case.cin, case.cout), (case.n, case.h, case.w, case.cout)
    if kind == "eighths":
        x = torch.randint(-4, 5, xs, generator=g).float()
        w = torch.randint(-2, 3, ws, generator=g).float() / 8
        dy = torch.randint(-2, 3, ys, generator=g).float()
        return x, w, dy, 0.125
    if kind == "sparse":
        # about 1.5 non-zero products per output: max |y| <= 15 with room to spare (asserted by the caller)
        d = min(1.0, (1.5 / (9.0 * case.cin)) ** 0.5)
        def tern(shape):
            return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float() * (torch.rand(shape, generator=g) < d).float()
        return tern(xs), tern(ws), tern(ys), 1.0
    x = torch.randn(xs, generator=g)
    w = torch.randn(ws, generator=g) / (9 * case.cin) ** 0.5
    dy = torch.randn(ys, generator=g)
    return x, w, dy, None


def reference(case, x, w, dy, rnd=None):
    """float64 y, dx, dw (on the CPU, or on the device for the big rows) and max(|x| conv |w|).  rnd: rounding of the
    intermediate tensors a reduced-precision tier stores (None here: the inputs are exact in bf16)."""
    dev = "cuda" if case.big else "cpu"
    x64 = x.to(dev).double().requires_grad_(True)
    w64 = w.to(dev).double().requires_grad_(True)
    y64 = tf_ops.conv_nd_same(x64, w64, dilation=case.dil)
    y64.backward(dy.to(dev).double())
    with torch.no_grad():
        amax = tf_ops.conv_nd_same(x64.abs(), w64.abs(), dilation=case.dil).max().item()
    return y64.detach(), x64.grad, w64.grad, amax


def _bf16_rne(t64):
    return t64.float().bfloat16()        # exact in fp32 first (asserted by the caller), then round-to-nearest-even


def _buffers(case, x, dy, prec):
    """Device operands of one precision: (x, dy, y buffer or None, dx buffer or None, guards).  Rows with xpad / ypad put x and
    dy into channel slices of wider poisoned buffers and have y / dx written into slices of sentinel-filled ones."""
    sd = torch.bfloat16 if prec == BF16S else torch.float32
    first = not (case.cin % 16 == 0 and case.cout % 32 == 0)
    xd = torch.float32 if first else sd
    xg, dyg = x.cuda().to(xd), dy.cuda().to(sd)
    guards = {}
    if prec != BF16S and (case.xpad or case.ypad):
        xo, yo = (case.xpad if case.xpad % 4 == 0 else 0), (case.ypad if case.ypad % 4 == 0 else 0)
        guards["x"] = guardbuf.guarded_input(xg, case.cin + case.xpad, xo)
        guards["dy"] = guardbuf.guarded_input(dyg, case.cout + case.ypad, yo)
        guards["y"] = guardbuf.guarded(dyg.shape, sd, case.cout + case.ypad, yo)
        if case.xpad % 4 == 0:
            guards["dx"] = guardbuf.guarded(xg.shape, sd, case.cin + case.xpad, xo)
        xg, dyg = guards["x"].view, guards["dy"].view
    return xg, dyg, guards


def run_row(ops, case, kind):
    """Every op of the row in every precision that admits it, exact inputs: names, statistic rows, bit equality."""
    assert kind in ("eighths", "sparse")
    x, w, dy, lsb = make_inputs(case, kind)
    y64, dx64, dw64, amax = reference(case, x, w, dy)
    npix = case.n * case.h * case.w
    # the exact regime: every partial sum of y / dx is a multiple of lsb below 2^24 lsb, and of dw a multiple of lsb_dw likewise
    assert amax / lsb < 2 ** 24, (amax, lsb)
    dmax = tf_ops.conv_nd_same(dy.abs().double(), w.abs().double().flip(0, 1).transpose(2, 3), dilation=case.dil).max().item() \
        if not case.big else 2.0 * 0.25 * 9 * case.cout
    assert dmax / lsb < 2 ** 24, (dmax, lsb)         # (big rows: the analytic worst case 9 Cout max|dy| max|w|, an upper bound of the computed one)
    assert 8 * npix < 2 ** 24, npix                    # |x dy| <= 8 (1 for the sparse set), one term per pixel and tap
    ymax = y64.abs().max().item()
    if kind == "sparse":
        assert ymax <= 15, ymax
    traced = TRACED.setdefault((case.id, kind), set())
    first = not (case.cin % 16 == 0 and case.cout % 32 == 0)
    tiers = [(FP32, (case.fwd, case.rows, case.dgrad, case.wgrad))]
    if case.bf16 is not None:
        tiers.append((BF16, case.bf16))
    if case.bf16s is not None:
        tiers.append((BF16S, case.bf16s))
    for prec, (e_fwd, e_rows, e_dgrad, e_wgrad) in tiers:
        tag = "{} {} {}".format(case.id, kind, PREC_NAME[prec])
        xg, dyg, guards = _buffers(case, x, dy, prec)
        wg = w.cuda()
        # ---- forward + statistic partials
        wp_f, wp_d = (wg, None) if first else ops.conv3x3_pack(wg, bf16=prec)
        yb = guards["y"].view if "y" in guards else None
        (y, stats, rows), names = _trace(ops, lambda: ops.conv3x3_fwd(xg, wp_f, case.cout, True, y=yb, bf16=prec, dilation=case.dil))
        _assert_trace(names, e_fwd, tag + " forward")
        traced.update(names)
        y_ref = y64.to(y.device)
        if prec == BF16S:
            assert torch.equal(y_ref.float().double(), y_ref)
            assert y.dtype == torch.bfloat16 and torch.equal(y, _bf16_rne(y_ref)), tag + " y"
        else:
            assert y.dtype == torch.float32 and torch.equal(y.double(), y_ref), tag + " y"
        assert rows == e_rows and tuple(stats.shape) == (2, rows, case.cout), (tag, rows, e_rows, tuple(stats.shape))
        stored_exact = prec != BF16S or torch.equal(_bf16_rne(y_ref).double(), y_ref)   # the sums are of what was stored
        if stored_exact:
            P = 256 if prec == FP32 else 512           # most pixels one statistic row covers on that path
            s64 = stats.double().sum(1)
            r1, r2 = y_ref.sum((0, 1, 2)), (y_ref * y_ref).sum((0, 1, 2))
            ex1 = P * ymax / lsb < 2 ** 24
            ex2 = P * ymax * ymax / (lsb * lsb) < 2 ** 24
            if ex1:
                assert torch.equal(s64[0], r1), tag + " sum y"
            else:
                assert ((s64[0] - r1).abs() <= 2e-4 * max(1.0, y_ref.abs().sum((0, 1, 2)).max().item())).all(), tag + " sum y"
            if ex2:
                assert torch.equal(s64[1], r2), tag + " sum y^2"
            else:
                assert ((s64[1] - r2).abs() <= 2e-5 * r2.abs()).all(), tag + " sum y^2"
            if ex1 and ex2:
                EXACT_STATS.setdefault(e_fwd[0], set()).add(case.id)
        if "y" in guards:
            assert guards["y"].check_untouched() and guards["y"].unwritten() == 0, tag + " y guard"
            assert guards["x"].changed_anywhere() == 0
        # ---- input gradient
        if e_dgrad is not None:
            dxb = guards["dx"].view if "dx" in guards else None
            dx, names = _trace(ops, lambda: ops.conv3x3_dgrad(dyg, wp_d, case.cin, dx=dxb, bf16=prec, dilation=case.dil))
            _assert_trace(names, e_dgrad, tag + " input gradient")
            traced.update(names)
            dx_ref = dx64.to(dx.device)
            if prec == BF16S:
                assert torch.equal(dx, _bf16_rne(dx_ref)), tag + " dx"
            else:
                assert torch.equal(dx.double(), dx_ref), tag + " dx"
            if "dx" in guards:
                assert guards["dx"].check_untouched() and guards["dx"].unwritten() == 0, tag + " dx guard"
                assert guards["dy"].changed_anywhere() == 0
        # ---- filter gradient, twice
        if e_wgrad is not None:
            dw, names = _trace(ops, lambda: ops.conv3x3_wgrad(xg, dyg, bf16=prec, dilation=case.dil))
            _assert_trace(names, e_wgrad, tag + " filter gradient")
            traced.update(names)
            assert torch.equal(dw.double(), dw64.to(dw.device)), tag + " dw"
            assert torch.equal(dw, ops.conv3x3_wgrad(xg, dyg, bf16=prec, dilation=case.dil)), tag + " dw twice"
    return traced


def test_table_ids_are_unique_and_plans_are_as_stated():
    L = lib()
    L.unetk_conv3x3_wgrad_ws_bytes.restype = ctypes.c_size_t
    assert len(BY_ID) == len(CASES)
    for rid, (S, S_bf16, _) in WG_PLANS.items():
        c = BY_ID[rid]
        assert (S_bf16 is not None) == (c.bf16 is not None), rid
        for prec, s_want, names in ((FP32, S, c.wgrad), (BF16, S_bf16, c.bf16[3] if c.bf16 else None)):
            if s_want is None:
                continue
            d = _desc(c.n, c.h, c.w, c.cin, c.cout, prec=prec, dil=c.dil)
            got = (L.unetk_conv3x3_wgrad_ws_bytes(ctypes.byref(d)) - 256) / (9.0 * c.cin * c.cout * 4)
            assert got == s_want, (rid, prec, got, s_want)
            red = [n for n in names if n.startswith("slab_reduce")]
            want = [] if s_want == 1 else ["slab_reduce_kernel<{}>".format(16 if s_want >= 64 else 4 if s_want >= 8 else 1)]
            assert red == want, (rid, prec, red, want)


@pytest.mark.parametrize("kind", ["eighths", "sparse"])
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_conv_paths_exact(ops, case, kind):
    run_row(ops, case, kind)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_conv_paths_gaussian_fp32(ops, case):
    """The bounds of test_gpu_ops.py, unchanged, on every row's path."""
    x, w, dy, _ = make_inputs(case, "gauss")
    y64, dx64, dw64, _ = reference(case, x, w, dy)
    first = not (case.cin % 16 == 0 and case.cout % 32 == 0)
    xg, wg, dyg = x.cuda(), w.cuda(), dy.cuda()
    wp_f, wp_d = (wg, None) if first else ops.conv3x3_pack(wg)

    def rel(a, b):
        b = b.to(a.device)
        return ((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()

    (y, stats, rows), names = _trace(ops, lambda: ops.conv3x3_fwd(xg, wp_f, case.cout, True, dilation=case.dil))
    _assert_trace(names, case.fwd, case.id + " forward")
    e = rel(y, y64)
    print(case.id, "y", e)
    assert e < GAUSS_Y_TOL.get(case.id, 2e-6), e
    yr = y64.to(y.device)
    s = stats.double().sum(1)
    assert ((s[0] - yr.sum((0, 1, 2))).abs() <= 2e-4 * max(1.0, yr.abs().sum((0, 1, 2)).max().item())).all()
    r2 = (yr * yr).sum((0, 1, 2))
    assert ((s[1] - r2).abs() <= 2e-5 * r2).all()
    if case.dgrad is not None:
        e = rel(ops.conv3x3_dgrad(dyg, wp_d, case.cin, dilation=case.dil), dx64)
        print(case.id, "dx", e)
        assert e < 3e-6, e
    if case.wgrad is not None:
        dw = ops.conv3x3_wgrad(xg, dyg, dilation=case.dil)
        e = rel(dw, dw64)
        print(case.id, "dw", e)
        assert e < (1e-5 if case.n * case.h * case.w >= 100000 else 3e-6), e
        assert torch.equal(dw, ops.conv3x3_wgrad(xg, dyg, dilation=case.dil))


ULP_BF16 = 2.0 ** -8


def _r(t):
    """the bf16 values a tensor rounds to (round to nearest even), as float64"""
    return t.float().bfloat16().double()


def _stored_ok(got_bf16, ref64, what, flips=2e-3):
    """test_gpu_bf16s.py's check of a bf16-stored result: every element within one bf16 ulp of the exact value, all but `flips`
    of them exactly its rounding."""
    got = got_bf16.double()
    err = (got - ref64).abs() / ref64.abs().clamp_min(1e-30)
    big = ref64.abs() > 1e-3 * ref64.abs().max()
    assert err[big].max().item() <= 1.01 * ULP_BF16, (what, err[big].max().item())
    exact = (got == _r(ref64))
    assert exact.double().mean().item() > 1.0 - flips, (what, exact.double().mean().item())


REDUCED = [(c, BF16) for c in CASES if c.bf16] + [(c, BF16S) for c in CASES if c.bf16s]


@pytest.mark.parametrize("case,prec", REDUCED, ids=["{}-{}".format(c.id, PREC_NAME[q]) for c, q in REDUCED])
def test_conv_paths_gaussian_reduced_precision(ops, case, prec):
    """Gaussian operands that bf16 does NOT hold exactly: the kernels' operand rounding and bf16 stores against float64 on
    round-to-nearest-even operands, with the bounds of test_gpu_bf16.py / test_gpu_bf16s.py."""
    expect = case.bf16 if prec == BF16 else case.bf16s
    e_fwd, e_rows, e_dgrad, e_wgrad = expect
    x, w, dy, _ = make_inputs(case, "gauss")
    if prec == BF16S:                               # activations are stored in bf16: the kernel's inputs are bf16 tensors
        x, dy = x.bfloat16().float(), dy.bfloat16().float()
    y64, dx64, dw64, _ = reference(case, _r(x).float(), _r(w).float(), _r(dy).float())
    sd = torch.bfloat16 if prec == BF16S else torch.float32
    xg, wg, dyg = x.cuda().to(sd), w.cuda(), dy.cuda().to(sd)
    wp_f, wp_d = ops.conv3x3_pack(wg, bf16=prec)
    big = case.n * case.h * case.w >= 100000

    def rel(a, b):
        b = b.to(a.device)
        return ((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()

    (y, stats, rows), names = _trace(ops, lambda: ops.conv3x3_fwd(xg, wp_f, case.cout, True, bf16=prec))
    _assert_trace(names, e_fwd, case.id + " forward")
    assert rows == e_rows
    yr = y64.to(y.device)
    s = stats.double().sum(1)
    r1, r2 = yr.sum((0, 1, 2)), (yr * yr).sum((0, 1, 2))
    if prec == BF16:
        e = rel(y, y64)
        print(case.id, "bf16 y", e)
        assert e < 3e-6, e
        assert ((s[0] - r1).abs() <= 3e-4 * max(1.0, yr.abs().sum((0, 1, 2)).max().item())).all()
        assert ((s[1] - r2).abs() <= 3e-5 * r2).all()
    else:
        _stored_ok(y, yr, case.id + " y")
        assert ((s[0] - r1).abs() < 3e-5 * yr.abs().sum((0, 1, 2)).max().item()).all()      # from the fp32 accumulators
        assert ((s[1] - r2).abs() / r2 < 3e-5).all()
    if e_dgrad is not None:
        dx, names = _trace(ops, lambda: ops.conv3x3_dgrad(dyg, wp_d, case.cin, bf16=prec))
        _assert_trace(names, e_dgrad, case.id + " input gradient")
        if prec == BF16:
            e = rel(dx, dx64)
            print(case.id, "bf16 dx", e)
            assert e < 3e-6, e
        else:
            _stored_ok(dx, dx64.to(dx.device), case.id + " dx")
    if e_wgrad is not None:
        dw, names = _trace(ops, lambda: ops.conv3x3_wgrad(xg, dyg, bf16=prec))
        _assert_trace(names, e_wgrad, case.id + " filter gradient")
        e = rel(dw, dw64)
        print(case.id, PREC_NAME[prec], "dw", e)
        if prec == BF16:
            assert e < (1e-5 if big else 5e-6), e
        else:
            assert e < (2e-5 if big else 1e-5), e
        assert torch.equal(dw, ops.conv3x3_wgrad(xg, dyg, bf16=prec))


def test_bf16s_tall_tile_with_a_4_channel_y_pad(ops):
    """UNETK_BF16S where the persistent kernel refuses the strides (y_stride % 8 != 0) but pick_bf16 still takes the 512 x 128
    tile (H >= 24, 200 blocks): conv3x3_igemm_bf16_kernel<4,2,4,2,true>, writing a channel slice of a wider bf16 buffer."""
    case = _c("bf16s_tall_ypad4", 25, 32, 128, 64, 128, 200, None, None, None, big=True)
    for kind in ("eighths", "sparse"):
        x, w, dy, lsb = make_inputs(case, kind)
        y64, _, _, amax = reference(case, x, w, dy)
        assert amax / lsb < 2 ** 24
        xg = x.cuda().bfloat16()
        wp_f, _ = ops.conv3x3_pack(w.cuda(), want_dgrad=False, bf16=BF16S)
        yb = guardbuf.guarded((case.n, case.h, case.w, case.cout), torch.bfloat16, case.cout + 4, 0)
        (y, stats, rows), names = _trace(ops, lambda: ops.conv3x3_fwd(xg, wp_f, case.cout, True, y=yb.view, bf16=BF16S))
        _assert_trace(names, ["conv3x3_igemm_bf16_kernel<4,2,4,2,true,false,false>"], kind)
        TRACED.setdefault((case.id, "eighths"), set()).update(names)
        assert rows == case.rows and tuple(stats.shape) == (2, rows, case.cout)
        assert torch.equal(y, y64.float().bfloat16()), kind
        assert yb.check_untouched() and yb.unwritten() == 0
        if kind == "sparse":
            assert y64.abs().max().item() <= 15
            s = stats.double().sum(1)
            assert torch.equal(s[0], y64.sum((0, 1, 2))) and torch.equal(s[1], (y64 * y64).sum((0, 1, 2)))
            EXACT_STATS.setdefault("conv3x3_igemm_bf16_kernel<4,2,4,2,true,false,false>", set()).add(case.id)


@pytest.mark.parametrize("cin", [1, 2, 3])
def test_bf16s_first_layer(ops, cin):
    """UNETK_BF16S first layer (fp32 image in, bf16 out): conv3x3_c3_mfma_kernel<Cin, bf16> forward and
    conv3x3_wgrad_c3_bf16s_kernel (9 Cin <= 32, Cout = 64; 8 tiles -> 8 splits -> slab_reduce_kernel<4>), exact inputs."""
    case = _c("bf16s_first_ci%d" % cin, 2, 13, 21, cin, 64, 8, None, None, None)
    for kind in ("eighths", "sparse"):
        x, w, dy, lsb = make_inputs(case, kind)
        y64, _, dw64, amax = reference(case, x, w, dy)
        assert amax / lsb < 2 ** 24 and 8 * case.n * case.h * case.w < 2 ** 24
        xg, dyg = x.cuda(), dy.cuda().bfloat16()
        (y, stats, rows), names = _trace(ops, lambda: ops.conv3x3_fwd(xg, w.cuda(), 64, True, bf16=BF16S))
        _assert_trace(names, ["conv3x3_c3_mfma_kernel<%d,unsignedshort,false>" % cin], kind)
        TRACED.setdefault((case.id, "eighths"), set()).update(names)
        assert rows == case.rows and y.dtype == torch.bfloat16
        assert torch.equal(y, y64.float().bfloat16().cuda()), kind
        assert tuple(stats.shape) == (2, rows, 64)
        if kind == "sparse":                       # |y| <= 15: exact in bf16 and in the fp32 sums either way
            assert y64.abs().max().item() <= 15
            s2 = stats.double().sum(1).cpu()
            assert torch.equal(s2[0], y64.sum((0, 1, 2))) and torch.equal(s2[1], (y64 * y64).sum((0, 1, 2)))
            EXACT_STATS.setdefault("conv3x3_c3_mfma_kernel<%d,unsignedshort,false>" % cin, set()).add(case.id)
        dw, names = _trace(ops, lambda: ops.conv3x3_wgrad(xg, dyg, bf16=BF16S))
        _assert_trace(names, ["conv3x3_wgrad_c3_bf16s_kernel(", "slab_reduce_kernel<4>"], kind)
        TRACED[(case.id, "eighths")].update(names)
        assert torch.equal(dw.double().cpu(), dw64), kind
        assert torch.equal(dw, ops.conv3x3_wgrad(xg, dyg, bf16=BF16S))


LEGACY_SHAPES = [       # rows of test_gpu_ops.py::CONV_SHAPES whose comments name the linear-pixel kernel: keep them true
    ((1, 8, 16, 64, 128), "conv3x3_igemm_lin_kernel<2,2,1,2,false,false,false,false,false,false>"),
    ((2, 24, 20, 32, 128), "conv3x3_igemm_lin_kernel<2,2,1,2,false,false,false,false,false,false>"),
    ((2, 24, 24, 48, 128), "conv3x3_igemm_lin_kernel<2,2,1,2,false,false,false,false,false,false>"),
    ((5, 12, 12, 64, 128), "conv3x3_igemm_kernel<2,2,1,2,1,1,0>"),
]


@pytest.mark.parametrize("shape,name", LEGACY_SHAPES)
def test_legacy_shapes_take_the_kernels_their_comments_name(ops, shape, name):
    n, h, w, cin, cout = shape
    x = torch.zeros((n, h, w, cin), device="cuda")
    wp_f, _ = ops.conv3x3_pack(torch.zeros((3, 3, cin, cout), device="cuda"))
    _, names = _trace(ops, lambda: ops.conv3x3_fwd(x, wp_f, cout, False))
    assert any(name in n_ for n_ in names), names


def _desc(n, h, w, cin, cout, xs=None, ys=None, prec=FP32, dil=1):
    from boxsegliver_amd import _abi
    return _abi.ConvDesc(n, h, w, cin, cout, xs or cin, ys or cout, prec, dil)


def _cd(a, b):
    return -(-a // b)


def sk_plan_bytes(n, h, w, cin, cout):
    """sk_plan's slab size for a 2-D forward (csrc/conv_igemm_lin.hip: lin_tune, lin_bm, sk_plan at their defaults), restated;
    0 = stream-K off.  Only called for shapes lin_ok admits.  It exists because the public query is the larger of the
    forward's and the input gradient's need, so "one unit short" of the query need not turn the forward's stream-K off.  A
    mismatch with the library shows as the `(need > 0) == on and query >= need` assertion or the "full" / "short" traces
    failing.  The plan's 1 GiB cap is not mirrored (no row comes near it)."""
    gpix = h * w
    lin, tiled = _cd(gpix, 128) * 128, _cd(h, 8) * 8 * _cd(w, 16) * 16
    tune = 3 if (lin * 10 > tiled * 9 and n * gpix >= 16 * 128) else 0
    eff = lambda b: b / float(_cd(b, 256) * 256)
    if cout % 128 != 0 or (tune & 1):
        bm = 128
    else:
        b128, b64 = n * _cd(gpix, 128) * (cout // 128), n * _cd(gpix, 64) * (cout // 128)
        bm = 64 if (b128 < 384 or eff(b64) * 0.95 > eff(b128)) else 128
    bn = 128 if (bm == 64 or cout % 128 == 0) else 64
    tiles, nc = n * _cd(gpix, bm) * (cout // bn), cin // 16
    if tiles >= 2048 or (tiles > 256 and eff(tiles) >= 0.92):
        return 0
    whole = 0 if tiles <= 256 else tiles // 256 * 256
    if (tune & 2) and tiles <= 1024:
        whole = 0
    rem = tiles - whole
    if whole > 0 and (rem < 128 or nc < 48):
        return 0
    if whole == 0 and tiles > 256 and nc < 48:
        return 0
    tot, G = rem * nc, 256
    if whole == 0 and tot >= 2048:
        G = 512
    while G > 32 and tot < G * 4:
        G >>= 1
    if tot < G * 4:
        return 0
    return rem * (_cd(nc, tot // G) + 1) * bm * bn * 4


@pytest.mark.parametrize("case", [c for c in CASES if c.sk], ids=[c.id for c in CASES if c.sk])
def test_stream_k_workspace_three_ways(ops, case):
    """unetk_conv3x3_fwd_ws with the workspace its stream-K plan needs, with none, and with one 16-byte unit less: the first
    traces the row's kernels (stream-K where sk_plan turns it on), the other two the plain kernel; all bit-equal to float64 and
    to each other.  unetk_conv3x3_ws_bytes (the larger of the forward's and the input gradient's need) must cover the plan."""
    L = lib()
    x, w, dy, lsb = make_inputs(case, "eighths")
    y64 = reference(case, x, w, dy)[0]
    xg = x.cuda()
    wp_f, _ = ops.conv3x3_pack(w.cuda())
    d = _desc(case.n, case.h, case.w, case.cin, case.cout)
    L.unetk_conv3x3_ws_bytes.restype = ctypes.c_size_t
    query = L.unetk_conv3x3_ws_bytes(ctypes.byref(d))
    need = sk_plan_bytes(case.n, case.h, case.w, case.cin, case.cout)
    on = any("lin_sk_fixup" in n for n in case.fwd)
    assert (need > 0) == on and query >= need, (need, query, on)
    plain = [case.fwd[0].replace("false,false,true,", "false,false,false,")]
    ws = guardbuf.GuardedWorkspace(need)
    ys = []
    for label, ptr, nbytes, expect in (("full", ws.ptr(), need, case.fwd), ("none", None, 0, plain),
                                       ("short", ws.ptr(), max(need - 16, 0), plain)):
        y = torch.full((case.n, case.h, case.w, case.cout), float("nan"), device="cuda")
        stats = torch.empty((2, case.rows, case.cout), device="cuda")
        rc, names = _trace(ops, lambda: L.unetk_conv3x3_fwd_ws(ctypes.byref(d), _p(xg), _p(wp_f), _p(y), _p(stats),
                                                              _p(ptr), ctypes.c_size_t(nbytes), _stream()))
        assert rc == 0, (label, rc)
        _assert_trace(names, expect, "{} {}".format(case.id, label))
        TRACED.setdefault((case.id, "eighths"), set()).update(names)
        assert torch.equal(y.double(), y64.to(y.device)), label
        assert ws.guard_intact(), label
        ys.append(y)
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


REFUSALS = [
    # what, entry point, (n, h, w, cin, cout, xs, ys, prec, dil), expected return code
    ("pack Cin % 4", "pack", (1, 8, 8, 6, 64, 0, 0, FP32, 1), E_UNSUPPORTED),
    ("pack Cout % 4", "pack", (1, 8, 8, 16, 30, 0, 0, FP32, 1), E_UNSUPPORTED),
    ("dgrad without an MFMA tile (Cin = 3)", "dgrad", (1, 8, 8, 3, 64, 4, 64, FP32, 1), E_UNSUPPORTED),
    ("dgrad without an MFMA tile (Cin = 16)", "dgrad", (1, 8, 8, 16, 64, 16, 64, FP32, 1), E_UNSUPPORTED),
    ("atrous forward Cin % 16", "fwd", (1, 8, 8, 8, 64, 8, 64, FP32, 2), E_UNSUPPORTED),
    ("atrous forward Cout % 64", "fwd", (1, 8, 8, 16, 32, 16, 32, FP32, 2), E_UNSUPPORTED),
    ("atrous filter gradient Cin % 64", "wgrad", (1, 8, 8, 32, 64, 32, 64, FP32, 2), E_UNSUPPORTED),
    ("dilation 3 forward", "fwd", (1, 8, 8, 16, 64, 16, 64, FP32, 3), E_UNSUPPORTED),
    ("dilation 3 input gradient", "dgrad", (1, 8, 8, 64, 64, 64, 64, FP32, 3), E_UNSUPPORTED),
    ("direct path Cout > 1024", "fwd", (1, 8, 8, 3, 1028, 3, 1028, FP32, 1), E_UNSUPPORTED),
    ("direct path LDS above 64 KiB (180 x Cin x 4 bytes)", "fwd", (1, 8, 8, 92, 4, 92, 4, FP32, 1), E_UNSUPPORTED),
    ("direct path Cout % 4", "fwd", (1, 8, 8, 3, 6, 3, 8, FP32, 1), E_UNSUPPORTED),
    ("filter gradient mode -1 (Cin = 7)", "wgrad", (1, 8, 8, 7, 64, 7, 64, FP32, 1), E_UNSUPPORTED),
    ("filter gradient workspace one byte short", "wgrad_short", (2, 16, 16, 64, 64, 64, 64, FP32, 1), E_WORKSPACE),
    ("forward x misaligned", "fwd_mis_x", (1, 8, 8, 16, 64, 16, 64, FP32, 1), E_BADARG),
    ("forward y misaligned", "fwd_mis_y", (1, 8, 8, 16, 64, 16, 64, FP32, 1), E_BADARG),
    ("input gradient dx misaligned", "dgrad_mis", (1, 8, 8, 64, 64, 64, 64, FP32, 1), E_BADARG),
    ("filter gradient dw misaligned", "wgrad_mis", (1, 8, 8, 64, 64, 64, 64, FP32, 1), E_BADARG),
    ("forward x_stride % 4 on an MFMA path", "fwd", (1, 8, 8, 16, 64, 18, 64, FP32, 1), E_BADARG),
]


@pytest.mark.parametrize("what,entry,shape,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(ops, what, entry, shape, code):
    """Every refusal is a host-side return before any launch: the expected code, an empty trace, outputs untouched."""
    L = lib()
    n, h, w, cin, cout, xs, ys, prec, dil = shape
    d = _desc(n, h, w, cin, cout, xs or cin, ys or cout, prec, dil)
    sent = 12345.0
    big = 9 * max(cin, 4) * max(cout, 4) + 64
    xbuf = torch.zeros(n * h * w * max(xs, cin) + 64, device="cuda")
    ybuf = torch.zeros(n * h * w * max(ys, cout) + 64, device="cuda")
    wbuf = torch.zeros(big, device="cuda")
    out = torch.full((max(xbuf.numel(), ybuf.numel(), big) + 64,), sent, device="cuda")
    out2 = torch.full((big,), sent, device="cuda")
    L.unetk_conv3x3_wgrad_ws_bytes.restype = ctypes.c_size_t
    if entry == "pack":
        call = lambda: L.unetk_conv3x3_pack(_p(wbuf), cin, cout, _p(out), _p(out2), _stream())
    elif entry == "fwd":
        call = lambda: L.unetk_conv3x3_fwd(ctypes.byref(d), _p(xbuf), _p(wbuf), _p(out), _p(out2), _stream())
    elif entry == "fwd_mis_x":
        call = lambda: L.unetk_conv3x3_fwd(ctypes.byref(d), _p(xbuf.data_ptr() + 4), _p(wbuf), _p(out), _p(out2), _stream())
    elif entry == "fwd_mis_y":
        call = lambda: L.unetk_conv3x3_fwd(ctypes.byref(d), _p(xbuf), _p(wbuf), _p(out.data_ptr() + 8), _p(out2), _stream())
    elif entry == "dgrad":
        call = lambda: L.unetk_conv3x3_dgrad(ctypes.byref(d), _p(ybuf), _p(wbuf), _p(out), _stream())
    elif entry == "dgrad_mis":
        call = lambda: L.unetk_conv3x3_dgrad(ctypes.byref(d), _p(ybuf), _p(wbuf), _p(out.data_ptr() + 4), _stream())
    else:
        nws = L.unetk_conv3x3_wgrad_ws_bytes(ctypes.byref(d))
        if entry == "wgrad":
            assert nws == 0 or dil != 1, nws       # an unsupported plan asks for no workspace
            nws = max(nws, 1 << 20)
        ws = torch.zeros(nws + 64, dtype=torch.uint8, device="cuda")
        give = nws - 1 if entry == "wgrad_short" else nws
        dwp = out.data_ptr() + (4 if entry == "wgrad_mis" else 0)
        call = lambda: L.unetk_conv3x3_wgrad(ctypes.byref(d), _p(xbuf), _p(ybuf), _p(dwp), _p(ws), ctypes.c_size_t(give), _stream())
    rc, names = _trace(ops, call)
    assert rc == code, (what, rc, code)
    assert names == [], names
    assert bool((out == sent).all()) and bool((out2 == sent).all())


@pytest.mark.parametrize("rid", ["t4_ragged", "lin_w3", "sk64"])
def test_bench_bracket_tag_is_the_first_traced_kernel(ops, rid):
    """With the profile brackets on, the forward bracket's tag is the name of the first launch inside it -- the tiled kernel,
    the linear-pixel kernel, and for a stream-K layer the linear kernel, not its fix-up; sk64 checks the input gradient too."""
    case = BY_ID[rid]
    x, w, dy, _ = make_inputs(case, "eighths")
    wp_f, wp_d = ops.conv3x3_pack(w.cuda())
    xg, dyg = x.cuda(), dy.cuda()
    expect = [case.fwd] + ([case.dgrad] if rid == "sk64" else [])
    recs = []
    ops.profile_begin(0)
    ops.profile_on(recs)
    try:
        ops.conv3x3_fwd(xg, wp_f, case.cout, True)
        if rid == "sk64":
            ops.conv3x3_dgrad(dyg, wp_d, case.cin)
    finally:
        ops.profile_on(None)
    torch.cuda.synchronize()
    names = [_norm(n) for n in ops.profile_read()[1]]
    assert len(recs) == len(expect), recs
    for (tag, _, i0, i1, _), kernels in zip(recs, expect):
        assert i1 - i0 == len(kernels), (tag, i0, i1)
        first = names[i0][4:] if names[i0].startswith("void") else names[i0]
        assert tag == first.split("(")[0] == kernels[0], (tag, names[i0], kernels)


def _names_of(ops, case, kind="eighths"):
    if (case.id, kind) not in TRACED:
        run_row(ops, case, kind)
    return TRACED[(case.id, kind)]


def test_every_stats_kernel_has_an_exactly_checked_row(ops):
    """Each forward kernel of the table (every precision) has a row whose sum y and sum y^2 were both compared exactly."""
    for case in CASES:
        for prec, e in ((FP32, case.fwd), (BF16, case.bf16 and case.bf16[0]), (BF16S, case.bf16s and case.bf16s[0])):
            if e and e[0] not in EXACT_STATS:
                run_row(ops, case, "sparse")
    missing = sorted({e[0] for case in CASES for e in (case.fwd, case.bf16 and case.bf16[0], case.bf16s and case.bf16s[0]) if e}
                     - set(EXACT_STATS))
    assert not missing, missing


def test_table_reaches_every_required_kernel(ops):
    """The union of the traced names over the table contains every entry of REQUIRED."""
    union = set()
    for case in CASES:
        union |= _names_of(ops, case)
    if ("bf16s_tall_ypad4", "eighths") not in TRACED:
        test_bf16s_tall_tile_with_a_4_channel_y_pad(ops)
    for cin in (1, 2, 3):
        if ("bf16s_first_ci%d" % cin, "eighths") not in TRACED:
            test_bf16s_first_layer(ops, cin)
    for key, names in TRACED.items():
        union |= names
    missing = [r for r in REQUIRED if not any(r in n for n in union)]
    assert not missing, missing
