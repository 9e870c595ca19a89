"""The transposed-conv family of csrc/deconv.hip (forward into the concat buffer, ReLU backward + bias gradient, input
gradient, filter gradient) on every dispatch path, with inputs for which fp32 and bf16 arithmetic is exact in any order.

Exact inputs: `x` integers in [-4, 4], `w` and `bias` eighths in [-1, 1], `dcat` integers in [-2, 2], the skip half of `cat`
arbitrary.  Every product is a multiple of 1/8 (1 for dw / db) and every partial sum is bounded by
    forward  8 (4 Cin + 1),   dx  8 * 2 * 4 kd Cout,   dw  8 M,   db  2 * 4 kd M        (M = N D H W input pixels)
units, all below 2^24 -- the largest rows have K = 4096 and M < 2^17, so 2^20 at most -- and all operands are exact in bf16.
run_row asserts the four bounds from the row's sizes, so a later row cannot silently leave the exact regime.  Whatever tile,
split or MFMA order a kernel uses, cat (up half), dx, dw, db then equal the float64 reference (oracle/tf_ops.conv_transpose_ks +
ReLU + concat + autograd) bit for bit: cast to float32 for UNETK_FP32 / UNETK_BF16; under UNETK_BF16S cat and dx are that value
rounded ONCE to bf16 (round to nearest even), dw and db float32.  ReLU ties: output channel 3 has a zero filter and a zero bias
and one input pixel in eight is zero, so cat == 0 on a large share of the elements; the reference's ReLU gradient at 0 is 0, the
masked gradient the kernel leaves in the workspace is compared with dcat * (cat > 0) element for element, and each row asserts
that it has ties under a non-zero dcat.

Each row of ROWS names the kernels it exists to reach: the GEMM tile of the forward and of the input gradient ("128" =
<2,2,2,2>, "256" = <2,2,4,2>, "64" = <4,1,1,2>; UNETK_BF16 / UNETK_BF16S have no 256-row tile) and the slab reducer of the
filter gradient per precision, written out by hand from pw_plan, deconv_plan, unetk_launch_slab_reduce and unetk_rows_reduce.  The
library's launch trace must show exactly those kernels in order (pack kernels excluded).  test_plans_are_as_stated ties the
splits S, tiles per split and bias-partial blocks of PLANS to the library through unetk_deconv*_bwd_ws_bytes, whose value is
a function of exactly those numbers.

What the dispatch code admits and what it cannot reach (UNREACHABLE below, each with its reason):
  * unetk_rows_reduce always takes rows_reduce_final_wide_kernel here: the bias partials have Cout % 4 == 0 columns, start 16-byte
    aligned and have at most UNETK_COL_BLOCKS = 1024 = UNETK_RR_WIDE_ROWS rows, so neither the first level nor the narrow final
    kernel can be launched by this family (the workspace still reserves the first level's 64 Cout floats above 256 rows).
  * the 64-column bf16 GEMM tile in the FORWARD: UNETK_BF16 needs Cout % 32 == 0 and UNETK_BF16S Cout % 64 == 0, so 4 Cout is
    always a multiple of 128.  The input gradient reaches it at Cin % 128 == 64.
  * a filter-gradient block with mb >= me: S = ceil(mtiles / tiles_per) leaves (S - 1) tiles_per <= mtiles - 1, so every split
    starts below M.
  * the early `break` of pw_epilogue: the row deltas 0..3, 8..11, 16..19, 24..27 of a lane ARE increasing in r, so the rows after
    the first one at or past M are all past M; rows m5 .. m29 have fragment rows on both sides of M.

Gaussian tier (same rows): the bounds of test_gpu_ops.py (cat 3e-6, dx / dw / db 5e-6), test_gpu_bf16.py (the same, against the
oracle's restatement of the bf16 arithmetic) and test_gpu_bf16s.py (stored values within one bf16 ulp, all but 2e-3 of them the
exact rounding; dw / db 1e-5), unchanged.  The backward is taken on the mask of the STORED forward value, as
test_gpu_bf16s.py does: at 10^7 outputs a pre-activation within fp32 rounding of zero exists, and the exact tier pins the mask.
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
CFG = {"128": "2,2,2,2", "256": "2,2,4,2", "64": "4,1,1,2"}
COL_BLOCKS, RR_DIRECT_ROWS = 1024, 256

Row = collections.namedtuple("Row", "id api n d h w cin cout kd fwd dgrad red bf16 bf16s coff stride bias dbias big")


def _r(id, api, n, d, h, w, cin, cout, kd, fwd, dgrad, red=None, bf16=False, bf16s=False, coff=None, stride=None, bias=None,
       dbias=None, big=False):
    coff = cout if coff is None else coff
    stride = 2 * cout if stride is None else stride
    bias = (api == "2d") if bias is None else bias
    dbias = (api == "2d") if dbias is None else dbias
    assert api in ("2d", "3d") and (api == "3d" or (d == 1 and kd == 1 and dbias))
    return Row(id, api, n, d, h, w, cin, cout, kd, fwd, dgrad, red, bf16, bf16s, coff, stride, bias, dbias, big)


# id, entry points, N, D, H, W, Cin, Cout, kd, forward tile, input-gradient tile (None: the backward refuses the shape),
#   red = slab reducer of the filter gradient (fp32, bf16, bf16s), which reduced precisions admit the row
ROWS = [
    # ---- GEMM tiles: forward N = 4 Cout columns, input gradient N = Cin columns
    _r("g128_small", "2d", 2, 1, 4, 8, 128, 64, 1, "128", "128", (1, 1, 1), bf16=True, bf16s=True),
    _r("fwd_co16", "3d", 1, 1, 3, 5, 16, 16, 1, "64", None),                 # 64 columns = four taps of 16 channels
    _r("fwd_co48_kd2", "3d", 1, 2, 2, 3, 32, 48, 2, "64", None),             # a 32-column fragment spans two taps
    _r("fwd_co80", "2d", 1, 1, 5, 3, 64, 80, 1, "64", None),
    _r("dg64_co32", "2d", 1, 1, 5, 3, 64, 32, 1, "128", "64", (1, 1, None), bf16=True),
    _r("dg64_ci192_kd2", "3d", 1, 2, 3, 2, 192, 64, 2, "128", "64", (1, 1, None), bf16=True),
    _r("dg64_ci320_co96", "2d", 2, 1, 3, 5, 320, 96, 1, "128", "64", (1, 1, None), bf16=True),
    _r("dg128_ci256", "2d", 2, 1, 8, 8, 256, 128, 1, "128", "128", (1, 1, 1), bf16=True, bf16s=True),
    # ---- planes narrower than a fragment, ragged M (fragment rows on both sides of M)
    _r("m1", "2d", 1, 1, 1, 1, 64, 64, 1, "128", "64", (1, 1, 1), bf16=True, bf16s=True),
    _r("m5_w5", "2d", 1, 1, 1, 5, 128, 64, 1, "128", "128", (1, 1, 1), bf16=True, bf16s=True),
    _r("m9_w3", "2d", 1, 1, 3, 3, 64, 128, 1, "128", "64", (1, 1, 1), bf16=True, bf16s=True),
    _r("m13_imgs", "2d", 13, 1, 1, 1, 128, 128, 1, "128", "128", (1, 1, 1), bf16=True, bf16s=True),
    _r("m21_w1", "2d", 3, 1, 7, 1, 64, 64, 1, "128", "64", (1, 1, 1), bf16=True, bf16s=True),
    _r("m29_w1", "2d", 1, 1, 29, 1, 192, 64, 1, "128", "64", (1, 1, 1), bf16=True, bf16s=True),
    _r("g3d_w2_kd2", "3d", 2, 3, 2, 2, 64, 32, 2, "128", "64", (1, 1, None), bf16=True),        # depth groups of 3 planes
    _r("m21_3d_kd2", "3d", 1, 7, 1, 3, 128, 64, 2, "128", "128", (1, 1, None), bf16=True),
    _r("m130", "2d", 2, 1, 5, 13, 128, 64, 1, "128", "128", (1, 1, 1), bf16=True, bf16s=True),
    _r("m300_w3", "2d", 4, 1, 25, 3, 64, 64, 1, "128", "64", (1, 1, 1), bf16=True, bf16s=True),
    # ---- relu_bwd_bias_kernel thread maps and grids, filter-gradient plans
    _r("co512", "2d", 1, 1, 2, 2, 64, 512, 1, "128", "64", (1, 1, 1), bf16=True, bf16s=True),
    _r("co1024", "2d", 1, 1, 2, 3, 64, 1024, 1, "128", "64", (1, 1, 1), bf16=True, bf16s=True),
    _r("nb300", "2d", 3, 1, 20, 20, 64, 64, 1, "128", "64", (4, 4, 4), bf16=True, bf16s=True),
    _r("cap_gridstride", "2d", 2, 1, 64, 65, 128, 64, 1, "128", "128", (16, 16, 16), bf16=True, bf16s=True),
    _r("multi_tile", "2d", 1, 1, 85, 150, 256, 256, 1, "128", "128", (4, 4, 4), bf16=True, bf16s=True, big=True),
    _r("wg_s5_tp3", "2d", 1, 1, 40, 40, 1024, 512, 1, "128", "128", (1, 1, 1), bf16=True, bf16s=True, big=True),
    # ---- the 256-row tile: K >= 1024 and ceil(M / 256) * n_ntiles >= 512, from both sides on both terms
    _r("f256_511", "2d", 1, 1, 100, 186, 1024, 224, 1, "128", "128", (4, 1, None), bf16=True, big=True),   # 73 x 7 = 511
    _r("f256_518", "2d", 1, 1, 100, 187, 1024, 224, 1, "256", "128", (4, 1, None), bf16=True, big=True),   # 74 x 7 = 518
    _r("fd256_512", "2d", 1, 1, 100, 162, 1024, 256, 1, "256", "256", (4, 1, 4), bf16=True, bf16s=True, big=True),   # 64 x 8
    _r("d256_511", "2d", 1, 1, 100, 186, 896, 256, 1, "128", "128", (4, 1, 4), bf16=True, bf16s=True, big=True),  # dgrad 73 x 7
    _r("f_k1008", "2d", 1, 1, 100, 162, 1008, 256, 1, "128", None, big=True),                                   # 512 blocks, K short
    # ---- concat geometry
    _r("geo_coff0", "2d", 2, 1, 3, 5, 64, 64, 1, "128", "64", (1, 1, 1), bf16=True, bf16s=True, coff=0, stride=64),
    _r("geo_three", "2d", 2, 1, 3, 5, 128, 64, 1, "128", "128", (1, 1, 1), bf16=True, bf16s=True, coff=36, stride=132),
    _r("geo_3d_bias", "3d", 1, 2, 2, 3, 64, 32, 2, "128", "64", (1, 1, None), bf16=True, coff=20, stride=60, bias=True, dbias=True),
]
BY_ID = {r.id: r for r in ROWS}

# deconv_plan per row and precision: (splits S, pixel tiles per split, blocks of relu_bwd_bias_kernel), written out by hand; tiles are
# 128 pixels, 64 for deconv_wgrad_bf16s4_kernel.  test_plans_are_as_stated checks them against the workspace query.
PLANS = {
    ("g128_small", FP32): (1, 1, 16),             # S = 1: one tile
    ("dg64_co32", FP32): (1, 1, 2),               # Cout = 32: 8 channel quads x 32 rows
    ("dg64_ci320_co96", FP32): (1, 1, 12),        # Cout = 96: 24 quads x 10 rows, 16 idle threads; ragged second co tile
    ("co512", FP32): (1, 1, 8),                   # 128 quads x 2 rows
    ("co1024", FP32): (1, 1, 24),                 # 256 quads x 1 row
    ("m130", FP32): (2, 1, 33),
    ("nb300", FP32): (10, 1, 300),                # more than 256 bias-partial rows
    ("nb300", BF16S): (10, 1, 300),
    ("cap_gridstride", FP32): (65, 1, 1024),      # S clamped by mtiles (384 -> 65); 2080 row groups on 1024 blocks: grid stride
    ("cap_gridstride", BF16): (65, 1, 1024),
    ("cap_gridstride", BF16S): (130, 1, 1024),
    ("multi_tile", FP32): (34, 3, 1024),          # 48 -> 34 (recomputed downwards); 33 splits of 3 tiles + one of 1, the last tile 78 px
    ("multi_tile", BF16): (15, 7, 1024),          # 14 splits of 7 + one of 2
    ("multi_tile", BF16S): (29, 7, 1024),         # 200 tiles of 64: 28 splits of 7 + one of 4
    ("wg_s5_tp3", FP32): (5, 3, 1024),            # 4 splits of 3 + one of 1, slab_reduce_kernel<1>
    ("wg_s5_tp3", BF16): (2, 7, 1024),
    ("wg_s5_tp3", BF16S): (4, 7, 1024),
    ("f256_511", FP32): (12, 13, 1024),           # Cout = 224: 56 quads x 4 rows, 32 idle threads
    ("fd256_512", FP32): (12, 11, 1024),
    ("fd256_512", BF16S): (8, 32, 1024),
    ("d256_511", FP32): (14, 11, 1024),
    ("d256_511", BF16): (5, 30, 1024),
    ("d256_511", BF16S): (10, 30, 1024),
    ("g3d_w2_kd2", FP32): (1, 1, 6),              # kd = 2: 8 M = 192 rows of 32 channels
}

REQUIRED = (["pw_gemm_kernel<%d,%s>" % (m, c) for m in (0, 1) for c in CFG.values()] +
            ["pw_gemm_bf16_kernel<0,2,2,2,2,false>", "pw_gemm_bf16_kernel<0,2,2,2,2,true>",
             "pw_gemm_bf16_kernel<1,2,2,2,2,false>", "pw_gemm_bf16_kernel<1,2,2,2,2,true>",
             "pw_gemm_bf16_kernel<1,4,1,1,2,false>", "pw_gemm_bf16_kernel<1,4,1,1,2,true>",
             "relu_bwd_bias_kernel<float>", "relu_bwd_bias_kernel<unsignedshort>", "rows_reduce_final_wide_kernel",
             "deconv_wgrad4_kernel", "deconv_wgrad_kernel<true>", "deconv_wgrad_bf16s_kernel", "deconv_wgrad_bf16s4_kernel",
             "slab_reduce_kernel<1>", "slab_reduce_kernel<4>", "slab_reduce_kernel<16>",
             "pack_deconv_kernel", "pack_deconv_bf16_kernel"])
UNREACHABLE = {
    "pw_gemm_bf16_kernel<0,4,1,1,2,false>": "UNETK_BF16 forward needs Cout % 32 == 0: 4 Cout is a multiple of 128",
    "pw_gemm_bf16_kernel<0,4,1,1,2,true>": "UNETK_BF16S forward needs Cout % 64 == 0: 4 Cout is a multiple of 128",
    "rows_reduce_l1_kernel": "at most 1024 bias-partial rows, float4-capable: the wide final kernel takes them directly",
    "rows_reduce_final_kernel": "Cout % 4 == 0 and a 16-byte aligned partial buffer: always the wide kernel",
}

TRACED = {}            # (row id, precision) -> set of traced kernel names (blanks removed)


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


def _cd(a, b):
    return -(-a // b)


def npix(row):
    return row.n * row.d * row.h * row.w


def fwd_ok(row, prec):
    """unetk_deconv3d_fwd's shape rules, restated."""
    if row.cin % 16 or row.cout % 16:
        return False
    if prec == BF16 and (row.cin % 32 or row.cout % 32):
        return False
    if prec == BF16S and (row.kd != 1 or row.cin % 64 or row.cout % 64 or row.stride % 2 or row.coff % 2):
        return False
    return True


def bwd_ok(row, prec):
    if row.cin % 64 or row.cout % 32 or row.cout > 1024 or row.stride % 4 or row.coff % 4:
        return False
    if prec == BF16S and (row.kd != 1 or row.cout % 64):
        return False
    return prec == FP32 or fwd_ok(row, prec)


def bf16s4(row, prec):
    return prec == BF16S and row.kd == 1 and row.cin % 128 == 0 and row.cout % 64 == 0


def plan(row, prec):
    """deconv_plan's filter-gradient splits and bias grid restated: (S, tiles per split, bias-partial blocks)."""
    M = npix(row)
    rpi = 256 // (row.cout // 4)
    nblk = min(_cd(4 * row.kd * M, rpi), COL_BLOCKS)
    if bf16s4(row, prec):
        panels, budget, tile = (row.cin // 128) * (row.cout // 64), 256, 64
    else:
        panels, budget, tile = (1 if prec == FP32 else 4) * (row.cin // 64) * _cd(row.cout, 64), (768 if prec == FP32 else 1024), 128
    mtiles = _cd(M, tile)
    S = max(1, min(_cd(budget, panels), mtiles))
    per = _cd(mtiles, S)
    return _cd(mtiles, per), per, nblk


def ws_bytes_of(row, S, nblk):
    """unetk_deconv3d_bwd_ws_bytes restated from (S, nblk)."""
    f = 4 * row.kd * npix(row) * row.cout + nblk * row.cout + (64 * row.cout if nblk > RR_DIRECT_ROWS else 0) + row.cout
    f = (f + 3) & ~3
    return (f + S * 4 * row.cin * row.cout) * 4


def reducer(S):
    return 16 if S >= 64 else 4 if S >= 8 else 1


def expected(row, prec):
    """(forward launches, backward launches of parts = 3, of parts = 1, of parts = 2) from the row's hand-written entries."""
    fk, dk = row.fwd, row.dgrad
    if prec != FP32:
        assert fk != "64"                                     # see UNREACHABLE
        fk, dk = ("128" if fk == "256" else fk), ("128" if dk == "256" else dk)
    tail = "" if prec == FP32 else (",true" if prec == BF16S else ",false")
    gemm = "pw_gemm_kernel" if prec == FP32 else "pw_gemm_bf16_kernel"
    fwd = ["{}<0,{}{}>".format(gemm, CFG[fk], tail)] * row.kd
    if dk is None or not bwd_ok(row, prec):
        return fwd, None, None, None
    relu = ["relu_bwd_bias_kernel<{}>".format("unsignedshort" if prec == BF16S else "float"), "rows_reduce_final_wide_kernel"]
    dg = "{}<1,{}{}>".format(gemm, CFG[dk], tail)
    wg = ("deconv_wgrad4_kernel" if prec == FP32 else "deconv_wgrad_kernel<true>" if prec == BF16 else
          "deconv_wgrad_bf16s4_kernel" if bf16s4(row, prec) else "deconv_wgrad_bf16s_kernel")
    red = "slab_reduce_kernel<{}>".format(row.red[prec])
    return fwd, relu + [dg, wg, red] * row.kd, relu + [dg] * row.kd, [wg, red] * row.kd


def make_inputs(row, kind, prec):
    """CPU float32 x [N,D,H,W,Cin], w [kd,2,2,Cout,Cin], bias [Cout] or None, the up half of dcat and the skip filler."""
    g = torch.Generator().manual_seed(9000 + sum(ord(ch) for ch in row.id) + (0 if kind == "exact" else 1))
    xs = (row.n, row.d, row.h, row.w, row.cin)
    ws = (row.kd, 2, 2, row.cout, row.cin)
    us = (row.n, row.kd * row.d, 2 * row.h, 2 * row.w, row.cout)
    if kind == "exact":
        x = torch.randint(-4, 5, xs, generator=g).float()
        if npix(row) >= 8:                                   # one input pixel in eight is zero: whole output pixels tie
            x = x * (torch.rand(xs[:-1], generator=g) >= 0.125).float().unsqueeze(-1)
        w = torch.randint(-8, 9, ws, generator=g).float() / 8
        w[:, :, :, 3, :] = 0                                 # output channel 3: zero filter, zero bias -> cat == 0 everywhere
        b = torch.randint(-8, 9, (row.cout,), generator=g).float() / 8
        b[3] = 0
        b[0::2] = 0                                          # and on the zero pixels for every even channel
        dup = torch.randint(-2, 3, us, generator=g).float()
    else:
        x = torch.randn(xs, generator=g)
        w = torch.randn(ws, generator=g) / row.cin ** 0.5
        b = 0.1 * torch.randn(row.cout, generator=g)
        dup = torch.randn(us, generator=g)
        if prec == BF16S:                                    # activations and their gradients ARE bf16 tensors in that mode
            x, dup = x.bfloat16().float(), dup.bfloat16().float()
    return x, w, (b if row.bias else None), dup


def reference(row, x, w, b, dup=None, rnd=None, dev="cpu"):
    """float64 pre-activation graph: returns (x64, w64, b64, pre).  rnd: rounding applied to x and w (UNETK_BF16 tier: the oracle's
    restatement conv_transpose_bf16_operands rounds by itself)."""
    x64 = x.to(dev).double().requires_grad_(True)
    w64 = w.to(dev).double().requires_grad_(True)
    b64 = b.to(dev).double().requires_grad_(True) if b is not None else None
    conv = tf_ops.conv_transpose_bf16_operands if rnd == "bf16" else tf_ops.conv_transpose_ks
    pre = conv(x64, w64, (row.kd, 2, 2), bias=b64)
    return x64, w64, b64, pre


class Call(object):
    """The device side of one row in one precision: guarded buffers and the C calls."""

    def __init__(self, row, prec, x, w, b, dup):
        from boxsegliver_amd import _abi
        self.row, self.prec, L = row, prec, lib()
        sd = torch.bfloat16 if prec == BF16S else torch.float32
        self.sd, self.esize = sd, (2 if prec == BF16S else 4)
        if row.api == "2d":
            self.desc = _abi.DeconvDesc(row.n, row.h, row.w, row.cin, row.cout, row.stride, row.coff, prec)
            self.fns = (L.unetk_deconv2x2_fwd, L.unetk_deconv2x2_bwd_ws_bytes, L.unetk_deconv2x2_bwd, L.unetk_deconv2x2_bwd_parts)
        else:
            self.desc = _abi.Deconv3dDesc(row.n, row.d, row.h, row.w, row.cin, row.cout, row.kd, row.stride, row.coff, prec)
            self.fns = (L.unetk_deconv3d_fwd, L.unetk_deconv3d_bwd_ws_bytes, L.unetk_deconv3d_bwd, L.unetk_deconv3d_bwd_parts)
        self.fns[1].restype = ctypes.c_size_t
        self.gx = guardbuf.guarded_input(x.cuda().to(sd))
        self.wg = w.cuda().contiguous()
        self.bg = guardbuf.guarded_input(b.cuda()) if b is not None else None
        ush = dup.shape
        self.gcat = guardbuf.guarded(ush, sd, row.stride, row.coff)
        gen = torch.Generator(device="cuda").manual_seed(5)
        pay = self.gcat.flat[self.gcat.guard:self.gcat.guard + self.gcat.payload]
        pay.copy_(torch.randn(pay.shape, device="cuda", generator=gen).to(sd))          # the skip half and whatever else the pixel holds
        self.gcat.bits()[self.gcat.mask] = guardbuf.SENTINEL[sd]
        self.gcat.snap = self.gcat.flat.clone()
        self.gdcat = guardbuf.guarded_input(dup.cuda().to(sd), row.stride, row.coff)
        self.gdx = guardbuf.guarded(x.shape, sd)
        self.gdw = guardbuf.guarded(w.shape)
        self.gdb = guardbuf.guarded((row.cout,)) if row.dbias else None
        self.wp_f = self.wp_d = None

    def base(self, g):
        return g.flat.data_ptr() + g.guard * self.esize

    def pack(self):
        row, L, prec = self.row, lib(), self.prec
        n = row.kd * 4 * row.cin * row.cout
        dt = torch.float32 if prec == FP32 else torch.bfloat16
        self.wp_f, self.wp_d = torch.empty(n, dtype=dt, device="cuda"), torch.empty(n, dtype=dt, device="cuda")
        if prec == FP32:
            return L.unetk_deconv3d_pack(_p(self.wg), row.kd, row.cin, row.cout, _p(self.wp_f), _p(self.wp_d), _stream())
        if prec == BF16:
            return L.unetk_deconv3d_pack_bf16(_p(self.wg), row.kd, row.cin, row.cout, _p(self.wp_f), _p(self.wp_d), _stream())
        return L.unetk_deconv2x2_pack_bf16s(_p(self.wg), row.cin, row.cout, _p(self.wp_f), _p(self.wp_d), _stream())

    def fwd(self):
        return self.fns[0](ctypes.byref(self.desc), _p(self.gx.view), _p(self.wp_f), _p(self.bg.view if self.bg else None),
                           _p(self.base(self.gcat)), _stream())

    def ws_query(self):
        return self.fns[1](ctypes.byref(self.desc))

    def bwd(self, ws, nbytes, parts=None):
        a = (ctypes.byref(self.desc), _p(self.gx.view), _p(self.wp_d), _p(self.base(self.gcat)), _p(self.base(self.gdcat)),
             _p(self.gdx.view), _p(self.gdw.view), _p(self.gdb.view if self.gdb else None), _p(ws.ptr()), ctypes.c_size_t(nbytes))
        if parts is None:
            return self.fns[2](*(a + (_stream(),)))
        return self.fns[3](*(a + (parts, _stream())))

    def outputs(self):
        return [g for g in (self.gdx, self.gdw, self.gdb) if g is not None]

    def out_bits(self):
        return [g.bits(g.view.contiguous()).clone() for g in self.outputs()]

    def inputs_intact(self, cat_after_fwd):
        return (self.gx.changed_anywhere() == 0 and self.gdcat.changed_anywhere() == 0 and
                (self.bg is None or self.bg.changed_anywhere() == 0) and torch.equal(self.gcat.bits(), self.gcat.bits(cat_after_fwd)))


ULP_BF16 = 2.0 ** -8


def _rb(t):
    return t.float().bfloat16().double()


def _stored_ok(got_bf16, ref64, what, flips=2e-3):
    """test_gpu_bf16s.py's check of a bf16-stored result: every element within one bf16 ulp of the exact value, all but `flips`
    of them exactly its rounding."""
    got = got_bf16.double()
    err = (got - ref64).abs() / ref64.abs().clamp_min(1e-30)
    big = ref64.abs() > 1e-3 * ref64.abs().max()
    assert err[big].max().item() <= 1.01 * ULP_BF16, (what, err[big].max().item())
    exact = (got == _rb(ref64))
    assert exact.double().mean().item() > 1.0 - flips, (what, exact.double().mean().item())


def _rel(a, b):
    b = b.to(a.device)
    return ((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def run_row(ops, row, prec, kind):
    exact = kind == "exact"
    M = npix(row)
    if exact:      # the exact regime (module docstring), from this row's sizes
        assert 8 * (4 * row.cin + 1) < 2 ** 24 and 8 * 2 * 4 * row.kd * row.cout < 2 ** 24, (row.cin, row.cout)
        assert 8 * M < 2 ** 24 and 2 * 4 * row.kd * M < 2 ** 24, M
    assert fwd_ok(row, prec)
    tag = "{} {} {}".format(row.id, PREC_NAME[prec], kind)
    e_fwd, e_bwd, e_p1, e_p2 = expected(row, prec)
    x, w, b, dup = make_inputs(row, kind, prec)
    dev = "cuda" if row.big else "cpu"
    rnd = "bf16" if (prec == BF16 and not exact) else None
    wr = w.bfloat16().float() if (prec == BF16S and not exact) else w
    x64, w64, b64, pre = reference(row, x, wr, b, rnd=rnd, dev=dev)
    up64 = torch.relu(pre).detach()
    c = Call(row, prec, x, w, b, dup)
    traced = TRACED.setdefault((row.id, prec), set())
    # ---- pack + forward into the guarded concat buffer
    rc, names = _trace(ops, c.pack)
    assert rc == 0, (tag, rc)
    traced.update(names)
    rc, names = _trace(ops, c.fwd)
    assert rc == 0, (tag, rc)
    _assert_trace(names, e_fwd, tag + " forward")
    traced.update(names)
    assert c.gcat.check_untouched(), tag + ": the skip half / the guards changed"
    assert c.gcat.unwritten() == 0, tag + ": up elements never written"
    assert c.gx.changed_anywhere() == 0
    cat = c.gcat.view
    upd = up64.to(cat.device)
    if exact:
        assert torch.equal(upd.float().double(), upd)
        if prec == BF16S:
            assert torch.equal(cat, upd.float().bfloat16()), tag + " cat"
        else:
            assert torch.equal(cat.double(), upd), tag + " cat"
        tie = upd == 0
        assert tie.any() and (dup.to(cat.device)[tie] != 0).any(), tag + ": no ReLU ties under a non-zero gradient"
    else:
        if prec == BF16S:
            _stored_ok(cat, upd, tag + " cat")
        else:
            e = _rel(cat, upd)
            print(tag, "cat", e)
            assert e < 3e-6, e
        assert (cat > 0).any() and (cat == 0).any() and (pre < 0).any(), tag
    if e_bwd is None:
        assert c.ws_query() == 0, tag + ": a refused backward asks for no workspace"
        return
    # ---- reference backward
    if exact:
        mask = (up64 > 0)
    else:
        mask = (cat.to(pre.device).double() > 0)                # the stored forward value's mask (module docstring)
    dpre64 = dup.to(pre.device).double() * mask
    grads = torch.autograd.grad(pre, [t for t in (x64, w64, b64) if t is not None], dpre64)
    dx64, dw64 = grads[0], grads[1]
    db64 = grads[2] if b64 is not None else dpre64.sum((0, 1, 2, 3))
    # ---- backward, twice, on a workspace of exactly the queried size filled with NaN patterns
    nbytes = c.ws_query()
    S, per, nblk = plan(row, prec)
    assert nbytes == ws_bytes_of(row, S, nblk), (tag, nbytes, S, per, nblk)
    assert row.red[prec] == reducer(S), (tag, S, row.red)
    ws = guardbuf.GuardedWorkspace(nbytes)
    cat_after = c.gcat.flat.clone()
    runs = []
    for rep in range(2):
        ws.fill(0xFF)
        for g in c.outputs():
            g.reset()
        rc, names = _trace(ops, lambda: c.bwd(ws, nbytes))
        assert rc == 0, (tag, rc)
        _assert_trace(names, e_bwd, tag + " backward")
        traced.update(names)
        assert ws.guard_intact(), tag + " workspace guard"
        for g in c.outputs():
            assert g.check_untouched() and g.unwritten() == 0, tag + " output guard"
        assert c.inputs_intact(cat_after), tag + ": an input changed"
        runs.append(c.out_bits())
    assert all(torch.equal(a, b_) for a, b_ in zip(runs[0], runs[1])), tag + ": two runs differ"
    dx, dw = c.gdx.view, c.gdw.view
    db = c.gdb.view if c.gdb is not None else None
    # the masked gradient the first part leaves at the head of the workspace: zero wherever cat == 0
    nd = 4 * row.kd * M * row.cout
    dpre = ws.buf[ws.off:ws.off + nd * c.esize].view(c.sd).double().reshape(dpre64.shape)
    assert torch.equal(dpre, dpre64.to(dpre.device)), tag + " masked gradient"
    assert not dpre[(cat == 0)].any(), tag + ": cat == 0 carries gradient"
    dxr, dwr, dbr = dx64.to(dx.device), dw64.to(dx.device), db64.to(dx.device)
    if exact:
        assert torch.equal(dxr.float().double(), dxr)
        if prec == BF16S:
            assert torch.equal(dx, dxr.float().bfloat16()), tag + " dx"
        else:
            assert torch.equal(dx.double(), dxr), tag + " dx"
        assert torch.equal(dw.double(), dwr), tag + " dw"
        if db is not None:
            assert torch.equal(db.double(), dbr), tag + " db"
    else:
        bound = 1e-5 if prec == BF16S else 5e-6
        if prec == BF16S:
            _stored_ok(dx, dxr, tag + " dx")
        else:
            e = _rel(dx, dxr)
            print(tag, "dx", e)
            assert e < bound, e
        e = _rel(dw, dwr)
        print(tag, "dw", e)
        assert e < bound, e
        if db is not None:
            e = _rel(db, dbr)
            print(tag, "db", e)
            assert e < bound, e
    # ---- parts 1 then parts 2 on the same stream and workspace: bit-equal to parts 3
    ws.fill(0xFF)
    for g in c.outputs():
        g.reset()
    rc, names = _trace(ops, lambda: c.bwd(ws, nbytes, 1))
    assert rc == 0, (tag, rc)
    _assert_trace(names, e_p1, tag + " parts 1")
    assert c.gdw.unwritten() == c.gdw.view.numel(), tag + ": parts 1 wrote dw"
    rc, names = _trace(ops, lambda: c.bwd(ws, nbytes, 2))
    assert rc == 0, (tag, rc)
    _assert_trace(names, e_p2, tag + " parts 2")
    assert ws.guard_intact() and c.inputs_intact(cat_after)
    for g in c.outputs():
        assert g.check_untouched(), tag + " output guard (parts)"
    assert all(torch.equal(a, b_) for a, b_ in zip(runs[0], c.out_bits())), tag + ": parts 1 + 2 differ from parts 3"


def precisions(row):
    return [FP32] + ([BF16] if row.bf16 else []) + ([BF16S] if row.bf16s else [])


RUNS = [(r, q) for r in ROWS for q in precisions(r)]
RUN_IDS = ["{}-{}".format(r.id, PREC_NAME[q]) for r, q in RUNS]


def test_table_is_consistent_with_the_dispatch_rules():
    """CPU-side checks of the table against the restated predicates of pw_plan and deconv_plan."""
    assert len(BY_ID) == len(ROWS)
    for row in ROWS:
        M = npix(row)
        assert row.bf16 == fwd_ok(row, BF16) and row.bf16s == fwd_ok(row, BF16S), row.id
        assert (row.dgrad is not None) == bwd_ok(row, FP32), row.id
        # pw_plan, forward: N = 4 Cout columns, K = Cin
        ncols, K = 4 * row.cout, row.cin
        want = "64" if ncols % 128 else ("256" if K >= 1024 and _cd(M, 256) * (ncols // 128) >= 512 else "128")
        assert row.fwd == want, (row.id, row.fwd, want)
        if row.dgrad is not None:                    # input gradient: N = Cin columns, K = 4 Cout
            ncols, K = row.cin, 4 * row.cout
            want = "64" if ncols % 128 else ("256" if K >= 1024 and _cd(M, 256) * (ncols // 128) >= 512 else "128")
            assert row.dgrad == want, (row.id, row.dgrad, want)
            for prec in precisions(row):
                if bwd_ok(row, prec):
                    assert row.red[prec] == reducer(plan(row, prec)[0]), (row.id, prec)
                else:
                    assert row.red[prec] is None, (row.id, prec)
    for (rid, prec), want in PLANS.items():
        assert plan(BY_ID[rid], prec) == want, (rid, prec, plan(BY_ID[rid], prec), want)
    # both sides of every cut-off are present
    assert {BY_ID[i].fwd for i in ("f256_511", "f256_518", "fd256_512", "f_k1008")} == {"128", "256"}
    assert (BY_ID["fd256_512"].dgrad, BY_ID["d256_511"].dgrad, BY_ID["f256_518"].dgrad) == ("256", "128", "128")
    nb = sorted({plan(r, FP32)[2] for r in ROWS if r.dgrad})
    assert nb[0] <= RR_DIRECT_ROWS < max(n for n in nb if n < COL_BLOCKS) and nb[-1] == COL_BLOCKS
    assert {r.cout for r in ROWS if r.dgrad} >= {32, 64, 96, 128, 256, 512, 1024}
    assert {r.cout for r in ROWS if r.fwd == "64"} >= {16, 48, 80}
    assert {r.cin for r in ROWS if r.dgrad == "64"} >= {64, 192, 320} and {r.cin for r in ROWS if r.dgrad == "128"} >= {128, 256}


def test_plans_are_as_stated():
    """unetk_deconv*_bwd_ws_bytes is a function of (S, bias-partial blocks): the hand-written plans hold in the library."""
    from boxsegliver_amd import _abi
    L = lib()
    L.unetk_deconv3d_bwd_ws_bytes.restype = ctypes.c_size_t
    for (rid, prec), (S, per, nblk) in PLANS.items():
        r = BY_ID[rid]
        d = _abi.Deconv3dDesc(r.n, r.d, r.h, r.w, r.cin, r.cout, r.kd, r.stride, r.coff, prec)
        assert L.unetk_deconv3d_bwd_ws_bytes(ctypes.byref(d)) == ws_bytes_of(r, S, nblk), (rid, prec)


@pytest.mark.parametrize("row,prec", RUNS, ids=RUN_IDS)
def test_deconv_paths_exact(ops, row, prec):
    run_row(ops, row, prec, "exact")


@pytest.mark.parametrize("row,prec", RUNS, ids=RUN_IDS)
def test_deconv_paths_gaussian(ops, row, prec):
    """The bounds of test_gpu_ops.py / test_gpu_bf16.py / test_gpu_bf16s.py, unchanged, on every row's path."""
    run_row(ops, row, prec, "gauss")


@pytest.mark.parametrize("rid,prec", [("g128_small", FP32), ("g128_small", BF16S), ("g3d_w2_kd2", FP32), ("g3d_w2_kd2", BF16)])
def test_workspace_16_bytes_short(ops, rid, prec):
    """UNETK_E_WORKSPACE before any launch: an empty trace, dx / dw / db untouched."""
    row = BY_ID[rid]
    x, w, b, dup = make_inputs(row, "exact", prec)
    c = Call(row, prec, x, w, b, dup)
    assert c.pack() == 0 and c.fwd() == 0
    nbytes = c.ws_query()
    ws = guardbuf.GuardedWorkspace(nbytes)
    for parts in (None, 1, 2, 3):
        rc, names = _trace(ops, lambda: c.bwd(ws, nbytes - 16, parts))
        assert rc == E_WORKSPACE and names == [], (parts, rc, names)
    for g in c.outputs():
        assert g.changed_anywhere() == 0
    assert torch.equal(ws.buf, ws.snap)


REFUSALS = [
    # what, call, (api, Cin, Cout, kd, out_stride, out_coff, precision), return code
    ("forward Cin % 16", "fwd", ("3d", 24, 32, 1, 64, 32, FP32), E_UNSUPPORTED),
    ("forward Cout % 16", "fwd", ("3d", 32, 24, 1, 48, 24, FP32), E_UNSUPPORTED),
    ("bf16 forward Cin % 32", "fwd", ("2d", 48, 32, 1, 64, 32, BF16), E_UNSUPPORTED),
    ("bf16 forward Cout % 32", "fwd", ("2d", 64, 48, 1, 96, 48, BF16), E_UNSUPPORTED),
    ("bf16s forward kd = 2", "fwd", ("3d", 64, 64, 2, 128, 64, BF16S), E_UNSUPPORTED),
    ("bf16s forward Cin % 64", "fwd", ("2d", 96, 64, 1, 128, 64, BF16S), E_UNSUPPORTED),
    ("bf16s forward Cout % 64", "fwd", ("2d", 64, 96, 1, 192, 96, BF16S), E_UNSUPPORTED),
    ("bf16s forward odd out_stride", "fwd", ("2d", 64, 64, 1, 129, 64, BF16S), E_UNSUPPORTED),
    ("bf16s forward odd out_coff", "fwd", ("2d", 64, 64, 1, 130, 65, BF16S), E_UNSUPPORTED),
    ("forward out_stride < out_coff + Cout", "fwd", ("2d", 64, 64, 1, 120, 64, FP32), E_BADARG),
    ("forward precision 3", "fwd", ("2d", 64, 64, 1, 128, 64, 3), E_BADARG),
    ("backward Cin % 64", "bwd", ("2d", 96, 64, 1, 128, 64, FP32), E_UNSUPPORTED),
    ("backward Cout % 32", "bwd", ("3d", 64, 48, 2, 96, 48, FP32), E_UNSUPPORTED),
    ("backward out_stride % 4", "bwd", ("2d", 64, 64, 1, 130, 64, FP32), E_UNSUPPORTED),
    ("backward out_coff % 4", "bwd", ("2d", 64, 64, 1, 132, 66, FP32), E_UNSUPPORTED),
    ("backward Cout > 1024", "bwd", ("2d", 64, 1056, 1, 2112, 1056, FP32), E_UNSUPPORTED),
    ("backward Cout > 1024, 3-D", "bwd", ("3d", 64, 2048, 2, 4096, 2048, FP32), E_UNSUPPORTED),
    ("bf16 backward Cout > 1024", "bwd", ("2d", 64, 1056, 1, 2112, 1056, BF16), E_UNSUPPORTED),
    ("bf16s backward kd = 2", "bwd", ("3d", 64, 64, 2, 128, 64, BF16S), E_UNSUPPORTED),
    ("bf16s backward Cout % 64", "bwd", ("2d", 64, 96, 1, 192, 96, BF16S), E_UNSUPPORTED),
    ("bf16s backward out_stride % 4", "bwd", ("2d", 64, 64, 1, 130, 64, BF16S), E_UNSUPPORTED),
    ("backward out_stride < out_coff + Cout", "bwd", ("2d", 64, 64, 1, 100, 64, FP32), E_BADARG),
    ("backward precision 3", "bwd", ("2d", 64, 64, 1, 128, 64, 3), E_BADARG),
    ("pack Cin % 4", "pack", ("3d", 6, 64, 1, 0, 0, FP32), E_UNSUPPORTED),
    ("pack Cout % 4", "pack", ("3d", 64, 6, 2, 0, 0, FP32), E_UNSUPPORTED),
    ("bf16 pack Cin % 8", "pack", ("3d", 36, 64, 1, 0, 0, BF16), E_UNSUPPORTED),
    ("bf16 pack Cout % 8", "pack", ("3d", 64, 36, 2, 0, 0, BF16), E_UNSUPPORTED),
    ("bf16s pack Cin % 64", "pack", ("2d", 96, 64, 1, 0, 0, BF16S), E_UNSUPPORTED),
    ("bf16s pack Cout % 64", "pack", ("2d", 64, 96, 1, 0, 0, BF16S), E_UNSUPPORTED),
]


@pytest.mark.parametrize("what,call,shape,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(ops, what, call, shape, code):
    """Every refusal is a host-side return before any launch: the expected code, an empty trace, outputs untouched, and a zero
    workspace query where the backward refuses."""
    from boxsegliver_amd import _abi
    L = lib()
    api, cin, cout, kd, stride, coff, prec = shape
    n, dd, h, w = 1, (2 if api == "3d" else 1), 2, 3
    sent = 12345.0
    nel = 4 * kd * n * dd * h * w * max(stride, 2 * cout, 2 * cin) + 4 * kd * cin * cout + 256
    src = torch.zeros(nel, device="cuda")
    outs = [torch.full((nel,), sent, device="cuda") for _ in range(4)]
    if api == "2d":
        d = _abi.DeconvDesc(n, h, w, cin, cout, stride, coff, prec)
        fwd_fn, ws_fn, bwd_fn, parts_fn = L.unetk_deconv2x2_fwd, L.unetk_deconv2x2_bwd_ws_bytes, L.unetk_deconv2x2_bwd, L.unetk_deconv2x2_bwd_parts
    else:
        d = _abi.Deconv3dDesc(n, dd, h, w, cin, cout, kd, stride, coff, prec)
        fwd_fn, ws_fn, bwd_fn, parts_fn = L.unetk_deconv3d_fwd, L.unetk_deconv3d_bwd_ws_bytes, L.unetk_deconv3d_bwd, L.unetk_deconv3d_bwd_parts
    ws_fn.restype = ctypes.c_size_t
    if call == "pack":
        if prec == FP32:
            calls = [lambda: L.unetk_deconv3d_pack(_p(src), kd, cin, cout, _p(outs[0]), _p(outs[1]), _stream())]
        elif prec == BF16:
            calls = [lambda: L.unetk_deconv3d_pack_bf16(_p(src), kd, cin, cout, _p(outs[0]), _p(outs[1]), _stream())]
        else:
            calls = [lambda: L.unetk_deconv2x2_pack_bf16s(_p(src), cin, cout, _p(outs[0]), _p(outs[1]), _stream())]
    elif call == "fwd":
        calls = [lambda: fwd_fn(ctypes.byref(d), _p(src), _p(src), _p(src), _p(outs[0]), _stream())]
    else:
        assert ws_fn(ctypes.byref(d)) == 0, what
        nb = ctypes.c_size_t(outs[3].numel() * 4)
        a = (ctypes.byref(d), _p(src), _p(src), _p(src), _p(src), _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]), nb)
        calls = [lambda: bwd_fn(*(a + (_stream(),)))] + [(lambda q: lambda: parts_fn(*(a + (q, _stream()))))(q) for q in (1, 2, 3)]
    for fn in calls:
        rc, names = _trace(ops, fn)
        assert rc == code, (what, rc, code)
        assert names == [], names
    assert all(bool((o == sent).all()) for o in outs)


def test_table_reaches_every_launchable_kernel(ops):
    """The union of the traced names over the table contains every entry of REQUIRED; REQUIRED and UNREACHABLE together are the
    kernels the family's entry points name (the instantiations of csrc/deconv.hip plus the shared reducers)."""
    for row, prec in RUNS:
        if (row.id, prec) not in TRACED:
            run_row(ops, row, prec, "exact")
    union = set()
    for names in TRACED.values():
        union |= names
    missing = [r for r in REQUIRED if not any(r in n for n in union)]
    assert not missing, missing
    reached = [u for u in UNREACHABLE if any(u in n for n in union)]
    assert not reached, reached
    known = REQUIRED + list(UNREACHABLE)
    strangers = sorted(n for n in union if not any(k in n for k in known))
    assert not strangers, strangers
